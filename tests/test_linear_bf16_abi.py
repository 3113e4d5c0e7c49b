"""Kernel-level parity of csrc/linear_bf16.hip through the C ABI (ctypes only: no routing predicate between the test and the
kernel), in the idiom of tests/test_gemm_abi.py: outputs are slices of sentinel-filled buffers, and two input families -- EXACT
(small integers, the fp32 result equals the fp64 reference bit for bit whatever the MFMA's summation order) and ROUND (seeded normal
inputs against fp64 on bf16-rounded operands, within the bound derived in tests/linear_bf16_cases.py).  The conversion is pinned by
known answers, alone and through the GEMM."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_cases as lc  # noqa: E402
from abi_harness import Arena, abi, place, same, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def to_bf16_device(t):
    """a host fp32 tensor -> device bf16 bits (int16 storage) by hf_f32_to_bf16"""
    _lib, L = abi()
    src = place(DEV, t)
    dst = torch.empty(t.numel() + 8, dtype=torch.int16, device=DEV)[:t.numel()].view(t.shape)
    _lib.check(L.hf_f32_to_bf16(t.numel(), _lib.ptr(src), _lib.ptr(dst), _lib.stream_ptr()), "hf_f32_to_bf16")
    return dst


def run(c, t):
    _lib, L = abi()
    ptr = _lib.ptr
    has_bn, mode, _ = lc.MODES[c["mode"]]
    a = Arena(DEV)
    x, wb, bias = place(DEV, t["x"]), to_bf16_device(t["w"]), place(DEV, t["bias"])
    bn = [place(DEV, v) for v in t["bn"]] if has_bn else [None] * 4
    y = a.out((c["rows"], c["cout"]))
    _lib.check(L.hf_linear_bf16_fwd_eval(c["rows"], c["cin"], c["cout"], ptr(x), ptr(wb), ptr(bias), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]),
                                         mode, ptr(y), _lib.stream_ptr()), "hf_linear_bf16_fwd_eval")
    a.check()
    return y


@pytest.mark.parametrize("c", lc.exact_cases(), ids=lc.case_id)
def test_exact_family_equals_fp64_bit_for_bit(c):
    t = lc.inputs(c)
    mode = lc.MODES[c["mode"]][1]
    ref = lc.reference(t, mode)
    if ref["pre"] is not None:
        assert float(ref["pre"].abs().min()) >= 1.0
    assert float(ref["y"].abs().max()) < 2 ** 24
    same(run(c, t), ref["y"].to(DEV), "y")


@pytest.mark.parametrize("c", lc.round_cases(), ids=lc.case_id)
def test_round_family_within_the_derived_bound(c):
    t = lc.inputs(c)
    mode = lc.MODES[c["mode"]][1]
    ref = lc.reference(t, mode)
    if ref["pre"] is not None:
        assert float(ref["pre"].abs().min()) >= lc.RELU_MARGIN
    within(run(c, t), ref["y"].to(DEV), ref["err"].to(DEV), lc.case_id(c))


def test_exact_family_has_a_case_with_more_workgroups_than_the_chip_holds():
    assert max(lc.workgroups(c["rows"], c["cout"]) for c in lc.exact_cases()) > lc.CU_RESIDENT_WORKGROUPS


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "dst_one_element_off"])
def test_conversion_known_answers(offset):
    """hf_f32_to_bf16 bit for bit against torch's CPU conversion: the vector body, the scalar tail (the count is no multiple of four)
    and, with the destination one element past an 8-byte boundary, the scalar form alone"""
    _lib, L = abi()
    vals = lc.conversion_values()
    assert vals.numel() % 4 != 0
    want = _bits(vals.to(torch.bfloat16))
    assert int(want[0]) == 0x3F81 and int(want[1]) == 0x3F80 and int(want[2]) == 0x3F82      # up, tie to even down, tie to even up
    src = place(DEV, vals)
    buf = torch.full((vals.numel() + 16,), 0x5555, dtype=torch.int16, device=DEV)
    dst = buf[8 + offset:8 + offset + vals.numel()]
    _lib.check(L.hf_f32_to_bf16(vals.numel(), _lib.ptr(src), _lib.ptr(dst), _lib.stream_ptr()), "hf_f32_to_bf16")
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), want), [(float(v), hex(int(g) & 0xffff), hex(int(w) & 0xffff)) for v, g, w in zip(vals, dst.cpu(), want) if g != w]
    assert bool((buf[:8 + offset] == 0x5555).all()) and bool((buf[8 + offset + vals.numel():] == 0x5555).all())


def test_conversion_inside_the_gemm():
    """the same values through the staging conversion: x = [v, 0, 0, 0], every weight row = [1, 0, 0, 0] -> y[r, :] = bf16(v) (the
    other products are 0 * 0; -0 + 0 = +0 compares equal to -0)"""
    _lib, L = abi()
    vals = lc.conversion_values()
    rows = vals.numel()
    x = torch.zeros(rows, 4)
    x[:, 0] = vals
    w = torch.zeros(4, 4)
    w[:, 0] = 1.0
    a = Arena(DEV)
    y = a.out((rows, 4))
    xd, wb = place(DEV, x), to_bf16_device(w)         # held until the call has run
    _lib.check(L.hf_linear_bf16_fwd_eval(rows, 4, 4, _lib.ptr(xd), _lib.ptr(wb), None, None, None, None, None, 0, _lib.ptr(y),
                                         _lib.stream_ptr()), "hf_linear_bf16_fwd_eval")
    a.check()
    want = vals.to(torch.bfloat16).float().view(rows, 1).expand(rows, 4)
    assert torch.equal(y.cpu(), want), (y.cpu()[:, 0].tolist(), want[:, 0].tolist())


def test_bad_arguments_are_rejected_on_the_device_too():
    _lib, L = abi()
    buf, out = torch.zeros(4096, device=DEV), torch.zeros(4096, device=DEV)
    p, off, q = _lib.ptr(buf), _lib.ptr(buf[1:]), _lib.ptr(out)
    call = lambda rows, cin, cout, x=p, w=p, y=q, bn=(None,) * 4, mode=0: L.hf_linear_bf16_fwd_eval(rows, cin, cout, x, w, None, *bn, mode, y,
                                                                                                   _lib.stream_ptr())
    assert call(8, 8, 8) == 0
    assert [call(0, 8, 8), call(8, 6, 8), call(8, 8, 6), call(8, 8, 8, x=off), call(8, 8, 8, w=off), call(8, 8, 8, y=_lib.ptr(out[1:])),
            call(8, 8, 8, mode=1), call(8, 8, 8, bn=(p, p, p, None)), call(8, 8, 8, bn=(p, p, p, p), mode=4)] == [_lib.HF_EINVAL] * 9
    torch.cuda.synchronize()
