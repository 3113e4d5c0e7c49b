"""Kernel-level parity of csrc/linear_bf16_train.hip through the C ABI (ctypes only: no routing predicate between the test and the
kernel), in the idiom of tests/test_linear_bf16_abi.py: outputs are slices of sentinel-filled buffers; the weight gradient in the
EXACT family (bit for bit against fp64) and the ROUND family (within the bound derived in tests/linear_bf16_train_cases.py); the
transposing conversion bit for bit against torch's CPU conversion; the input gradient as the composition of the transposing
conversion and hf_linear_bf16_fwd_eval."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_train_cases as tc  # noqa: E402
from abi_harness import Arena, abi, place, same, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def run_wgrad(c, t):
    """-> dW; the workspace is a slice of a sentinel-filled buffer as well, of exactly the size the query names"""
    _lib, L = abi()
    ptr = _lib.ptr
    a = Arena(DEV)
    g, x = place(DEV, t["g"]), place(DEV, t["x"])
    nbytes = L.hf_linear_bf16_wgrad_workspace(c["rows"], c["cout"], c["cin"])
    tiles, rpc, chunks = tc.plan(c["rows"], c["cout"], c["cin"])
    assert nbytes == 4 * chunks * c["cout"] * c["cin"], "the plan restated in linear_bf16_train_cases.py is not the library's"
    ws = a.out((nbytes // 4,))
    dw = a.out((c["cout"], c["cin"]))
    _lib.check(L.hf_linear_bf16_wgrad(c["rows"], c["cout"], c["cin"], ptr(g), ptr(x), ptr(dw), ptr(ws), nbytes, _lib.stream_ptr()),
               "hf_linear_bf16_wgrad")
    a.check()
    return dw


@pytest.mark.parametrize("c", tc.exact_cases(), ids=tc.case_id)
def test_wgrad_exact_family_equals_fp64_bit_for_bit(c):
    t = tc.inputs(c)
    ref = tc.reference(t)
    assert float(ref["dw"].abs().max()) < 2 ** 24
    same(run_wgrad(c, t), ref["dw"].to(DEV), "dW")


@pytest.mark.parametrize("c", tc.round_cases(), ids=tc.case_id)
def test_wgrad_round_family_within_the_derived_bound(c):
    t = tc.inputs(c)
    ref = tc.reference(t)
    within(run_wgrad(c, t), ref["dw"].to(DEV), ref["err"].to(DEV), tc.case_id(c))


def test_exact_family_has_a_case_with_more_workgroups_than_the_chip_holds():
    assert max(tc.workgroups(c["rows"], c["cout"], c["cin"]) for c in tc.exact_cases()) > tc.CU_RESIDENT_WORKGROUPS


@pytest.mark.parametrize("c", [tc.round_cases()[1], tc.round_cases()[2]], ids=tc.case_id)
def test_two_calls_give_the_same_bits(c):
    t = tc.inputs(c)
    assert tc.plan(c["rows"], c["cout"], c["cin"])[2] > 1
    first, second = run_wgrad(c, t), run_wgrad(c, t)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))


def run_transpose(src):
    """-> dst (cols, rows) int16 bits, a slice of a buffer filled with 0x5555 whose two sides are checked"""
    _lib, L = abi()
    rows, cols = src.shape
    s = place(DEV, src)
    buf = torch.full((rows * cols + 16,), 0x5555, dtype=torch.int16, device=DEV)
    dst = buf[8:8 + rows * cols]
    _lib.check(L.hf_f32_to_bf16_transpose(rows, cols, _lib.ptr(s), _lib.ptr(dst), _lib.stream_ptr()), "hf_f32_to_bf16_transpose")
    torch.cuda.synchronize()
    assert bool((buf[:8] == 0x5555).all()) and bool((buf[8 + rows * cols:] == 0x5555).all()), "write outside dst"
    return dst.view(cols, rows)


@pytest.mark.parametrize("shape", tc.transpose_cases(), ids=lambda s: "%dx%d" % s)
def test_transposing_conversion_equals_torch_bit_for_bit(shape):
    src = tc.transpose_input(*shape)
    assert torch.equal(run_transpose(src).cpu(), tc.transpose_reference_bits(src))


def test_transposing_conversion_known_answers():
    m = tc.conversion_matrix()
    want = tc.transpose_reference_bits(m)
    assert [int(v) & 0xffff for v in want[1, :3]] == [0x3F81, 0x3F80, 0x3F82]      # up, tie to even down, tie to even up
    got = run_transpose(m).cpu()
    assert torch.equal(got, want), [(float(v), hex(int(a) & 0xffff), hex(int(b) & 0xffff)) for v, a, b in zip(m[:, 1], got[1], want[1]) if a != b]


@pytest.mark.parametrize("shape", tc.dx_cases(), ids=lambda s: "%dx%dx%d" % s)
def test_input_gradient_as_a_composition_equals_fp64(shape):
    """dx (rows, cin) = g W: W (cout, cin) -> Wt_bf16 (cin, cout) by the transposing conversion, then the forward tile machine with the
    roles of cin and cout swapped; small integers, so the result equals fp64 bit for bit"""
    _lib, L = abi()
    ptr = _lib.ptr
    rows, cout, cin = shape
    t = tc.dx_inputs(rows, cout, cin)
    wt = run_transpose(t["w"])                       # (cin, cout), 16-byte aligned: eight int16 into the buffer
    assert wt.data_ptr() % 16 == 0
    a = Arena(DEV)
    g = place(DEV, t["g"])
    dx = a.out((rows, cin))
    _lib.check(L.hf_linear_bf16_fwd_eval(rows, cout, cin, ptr(g), ptr(wt), None, None, None, None, None, 0, ptr(dx), _lib.stream_ptr()),
               "hf_linear_bf16_fwd_eval")
    a.check()
    same(dx, (t["g"].double() @ t["w"].double()).to(DEV), "dx")


def test_bad_arguments_are_rejected_on_the_device_too():
    _lib, L = abi()
    E = _lib.HF_EINVAL
    buf, out, ws = torch.zeros(4096, device=DEV), torch.zeros(4096, device=DEV), torch.zeros(4096, device=DEV)
    p, q, w = _lib.ptr(buf), _lib.ptr(out), _lib.ptr(ws)
    need = L.hf_linear_bf16_wgrad_workspace(8, 8, 8)
    assert need == 4 * 8 * 8

    def wg(rows=8, cout=8, cin=8, g=p, x=p, dw=q, work=w, nbytes=need):
        return L.hf_linear_bf16_wgrad(rows, cout, cin, g, x, dw, work, nbytes, _lib.stream_ptr())

    assert wg() == 0
    assert [wg(rows=0), wg(cout=6), wg(cin=6), wg(g=_lib.ptr(buf[1:])), wg(x=_lib.ptr(buf[1:])), wg(dw=_lib.ptr(out[1:])), wg(work=None),
            wg(work=_lib.ptr(ws[1:])), wg(nbytes=need - 4), wg(g=None), wg(x=None), wg(dw=None)] == [E] * 12
    half = buf.view(torch.int16)
    tr = lambda rows=8, cols=8, src=p, dst=q: L.hf_f32_to_bf16_transpose(rows, cols, src, dst, _lib.stream_ptr())
    assert tr() == 0
    assert [tr(rows=0), tr(cols=0), tr(src=None), tr(dst=None), tr(src=_lib.ptr(half[1:])), tr(dst=_lib.ptr(out.view(torch.int8)[1:]))] == [E] * 6
    torch.cuda.synchronize()
    assert bool((out[64:] == 0).all()) and bool((ws == 0).all())       # one chunk: dW written directly, the workspace untouched
