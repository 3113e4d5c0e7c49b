"""hf_onepass_lift_elu_bn_bwd (csrc/lift_bwd.hip) through the C ABI: the lifting chain's backward with dy0 = dz1 W1 formed once.
Inputs are the lifting cases' own (tests/gemm_runs.lift_inputs, seeded by gemm_cases), the reference is fp64 autograd
(gemm_cases.ref_lift_bwd_autograd) and the bounds are gemm_cases.lift_bwd_bounds with this kernel's chain lengths: the grid, the
tile walk and col_sums_store are those of lift_linear_bwd_kernel, so a lane adds 16 rows per tile and tile of its workgroup, then the
other row-half and the four waves: 16 * tiles_per_workgroup + 4.

Why the two-pass bound of grad_w0 holds for the one-pass form without a further term.  The kernel sums, per channel c and d = 0, 1, 2,
  A_d = sum_r v (s x_d),   B_d = sum_r s x_d,   C_d = sum_r xhat (s x_d)          (v = dy0, s = elu'(z0), in fp32 per workgroup)
and the finalize evaluates  dW0[c][d] = a_c (A_d - (dbeta_c / R) B_d - (dgamma_c / R) C_d)  in fp64 from fp64 sums over the workgroups,
rounded once (the bound's trailing u |grad_w0|).  lift_bwd_bounds charges every row r
  |x_d| ( (10 + chain + 1) u Z_r s_r + |a| s_r (c1 u D_r + d_dbeta / R + X_r d_dgamma / R + err_x |dgamma| / R) + Z_r err_s ),
  Z_r = |a| (|v_r| + |dbeta| / R + X_r |dgamma| / R),   X_r >= |xhat_r|.
The three sums' own errors fall under the three terms of Z_r one by one:
  A_d: 2 products + a chain of adds on |v_r| s_r |x_d|, v_r carrying c1 u D_r, s_r carrying err_s   -> (chain + 2) u |a| |v_r| s_r |x_d| + ...
  B_d: 1 product + the chain on s_r |x_d|, scaled by |a| |dbeta| / R                                 -> (chain + 1) u |a| |dbeta| / R s_r |x_d| + ...
  C_d: 2 products + the chain on |xhat_r| s_r |x_d| (xhat_r carrying err_x), scaled by |a| |dgamma| / R -> (chain + 2) u |a| X_r |dgamma| / R s_r |x_d| + ...
and the fp64 sums S1, S2 that stand for dbeta, dgamma are within d_dbeta, d_dgamma of the reference's (they are those outputs before
their rounding), which is the |a| s_r (d_dbeta / R + X_r d_dgamma / R) term.  The fp64 arithmetic of the finalize adds nothing at this
scale.  At most chain + 2 < 10 + chain + 1 roundings per term: no term is missing, no factor is fitted.

grad_w1, dgamma0 and dbeta0 must equal hf_lift_elu_bn_bwd's bit for bit: dW1 is the same two launches; the two sums are formed by
the same expressions in the same order on the same grid, and the finalize adds the workgroups in bn_reduce_channel's order.

Run as a script (on a GPU), the module prints profiles/lift_bwd_onepass_parity.md."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402
from abi_harness import SENTINEL, Arena, abi, call, place, within  # noqa: E402
from gemm_runs import UNSET, lift_inputs, run_lift_bwd  # noqa: E402
from lift_bwd_cases import CASES, MAX_C0, TWINS, instantiations  # noqa: E402

pytestmark = pytest.mark.gpu

DEV, EPS = "cuda", 1e-3


def run_onepass(c, t, stats, short_by=0):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, c0, c1, mis = c["rows"], c["c0"], c["c1"], c["misalign"]
    a = Arena(DEV)
    x3, w0, g0, b0 = place(DEV, t["x3"]), place(DEV, t["w0"]), place(DEV, t["bn0"][0]), place(DEV, t["bn0"][1])
    mean0, invstd0 = place(DEV, stats[0]), place(DEV, stats[1])
    dz1, w1t = place(DEV, t["dz1"], mis == "dz1"), place(DEV, t["w1"].t().contiguous(), mis == "w1_t")
    gw0t, gw1, dg0, db0 = a.out((3, c0)), a.out((c1, c0)), a.out((c0,)), a.out((c0,))
    nbytes = L.hf_onepass_lift_elu_bn_bwd_workspace(rows, c0, c1)
    ws = a.out((nbytes // 4,))
    status = L.hf_onepass_lift_elu_bn_bwd(rows, c0, c1, ptr(x3), ptr(w0), ptr(g0), ptr(b0), ptr(mean0), ptr(invstd0), ptr(dz1), ptr(w1t),
                                          ptr(gw0t), ptr(gw1), ptr(dg0), ptr(db0), ptr(ws), nbytes - short_by, sp)
    a.check()
    out = dict(grad_w0_t=gw0t, grad_w1=gw1, dgamma0=dg0, dbeta0=db0)
    if short_by:
        return status, out
    call(status, "hf_onepass_lift_elu_bn_bwd")
    return out


def measure(c):
    """-> (outputs of the one-pass entry, outputs of the two-pass entry, {output: (|got - ref64|, bound)})"""
    t = lift_inputs(c)
    dv = lambda v: v.to(DEV)
    rows, c0, c1 = c["rows"], c["c0"], c["c1"]
    gw1, gg0, gb0, gw0, mean, invstd = gc.ref_lift_bwd_autograd(dv(t["x3"]), dv(t["w0"]), dv(t["bn0"][0]), dv(t["bn0"][1]), dv(t["w1"]), dv(t["dz1"]), EPS)
    stats = (mean.float(), invstd.float())
    got, old = run_onepass(c, t, stats), run_lift_bwd(c, t, stats)
    _, _, rpc, chunks = gc.wgrad_plan(rows, c1, c0)
    b = gc.lift_bwd_bounds(dv(t["x3"]), dv(t["w0"]), [dv(t["bn0"][0]), dv(t["bn0"][1]), mean, invstd], dv(t["w1"]), dv(t["dz1"]),
                           16 * gc.tiles_per_workgroup(rows, gc.cdiv(c0, 32)) + 4, min(rows, rpc) + gc.cdiv(chunks, 16) + 15)
    ref = dict(grad_w1=(gw1, b["d_w1"]), dbeta0=(gb0, b["d_dbeta"]), dgamma0=(gg0, b["d_dgamma"]), grad_w0_t=(gw0.t(), b["d_w0"].t()))
    return got, old, ref


@pytest.mark.parametrize("c", CASES, ids=gc.case_id)
def test_onepass_against_fp64_autograd_and_the_two_pass_entry(c):
    got, old, ref = measure(c)
    for name in ("grad_w1", "dbeta0", "dgamma0", "grad_w0_t"):
        within(got[name], ref[name][0], ref[name][1], name)
    for name in ("grad_w1", "dgamma0", "dbeta0"):
        assert torch.equal(got[name], old[name]), "%s differs from hf_lift_elu_bn_bwd" % name


def _run(c):
    t = lift_inputs(c)
    return run_onepass(c, t, (t["bn0"][2], t["bn0"][3]))


@pytest.mark.parametrize("c", TWINS, ids=gc.case_id)
def test_operand_one_float_off_a_16_byte_boundary(c):
    """the scalar twin stages the same values: every output is bit-identical to the aligned call"""
    assert instantiations(c) != instantiations(dict(c, misalign=None))
    off, aligned = _run(c), _run(dict(c, misalign=None))
    for k in aligned:
        assert torch.equal(off[k], aligned[k]), k


def test_two_calls_give_the_same_bits():
    c = gc._case("lift_bwd", rows=40000, c0=96, c1=100, family="round")
    first, second = _run(c), _run(c)
    for k in first:
        assert torch.equal(first[k], second[k]), k


def test_limits_and_a_short_workspace_are_rejected_before_anything_is_launched():
    _lib, L = abi(UNSET)
    sp = _lib.stream_ptr()
    buf = torch.zeros(16 * 16384, device=DEV)
    buf[8 * 16384:9 * 16384] = 1.0
    q = lambda i: _lib.ptr(buf[i * 16384:])
    poison = torch.full((4, 16384), SENTINEL, device=DEV)                  # grad_w0_t, grad_w1, dgamma0, dbeta0
    o = lambda i: _lib.ptr(poison[i])
    wsb = torch.full((1 << 22,), SENTINEL, device=DEV)
    ws, n = _lib.ptr(wsb), wsb.numel() * 4
    rows = 8
    f = lambda c0, c1=32, x=q(0), ws=ws, n=n: L.hf_onepass_lift_elu_bn_bwd(rows, c0, c1, x, q(9), q(8), q(5), q(5), q(8), q(10), q(1), o(0), o(1), o(2),
                                                                           o(3), ws, n, sp)
    need = L.hf_onepass_lift_elu_bn_bwd_workspace(rows, 36, 32)
    assert need == L.hf_linear_wgrad_workspace(rows, 32, 36) + 4 * 11 * 36 * gc.BN_MAX_BLOCKS
    got = [f(6), f(MAX_C0 + 4), f(0), f(36, 257), f(36, 0), f(36, x=None), f(36, ws=None), f(36, n=need - 1)]
    assert got == [_lib.HF_EINVAL] * 6 + [_lib.HF_EWORKSPACE] * 2
    torch.cuda.synchronize()
    assert bool((poison == SENTINEL).all()) and bool((wsb == SENTINEL).all()), "a rejected call wrote something"
    assert f(MAX_C0) == 0 and f(36, n=need) == 0                              # the limit itself and the exact workspace are accepted
    torch.cuda.synchronize()
    c = gc._case("lift_bwd", rows=300, c0=36, c1=100, family="round")
    t = lift_inputs(c)
    status, out = run_onepass(c, t, (t["bn0"][2], t["bn0"][3]), short_by=1)
    assert status == _lib.HF_EWORKSPACE
    assert all(bool((v == SENTINEL).all()) for v in out.values())


def render():
    lines = ["# Parity of hf_onepass_lift_elu_bn_bwd with fp64 autograd through the C ABI", "",
             "max |got - ref64| / bound per output (bounds: `gemm_cases.lift_bwd_bounds`, see `tests/test_lift_bwd_onepass_abi.py`), and the same",
             "ratio of the two-pass entry `hf_lift_elu_bn_bwd` for grad_w0_t on the same inputs; produced by",
             "`python tests/test_lift_bwd_onepass_abi.py` on an MI355X.", "",
             "| rows | c0 | c1 | grad_w1 | dbeta0 | dgamma0 | grad_w0_t | grad_w0_t, two-pass |", "|---:|---:|---:|---:|---:|---:|---:|---:|"]
    worst = {}
    for c in CASES:
        got, old, ref = measure(c)
        ratio = lambda out, name: float(((out[name].double() - ref[name][0]).abs() / ref[name][1].clamp(min=1e-300)).max())
        r = {name: ratio(got, name) for name in ("grad_w1", "dbeta0", "dgamma0", "grad_w0_t")}
        r["two"] = ratio(old, "grad_w0_t")
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        lines.append("| %d | %d | %d | %.3g | %.3g | %.3g | %.3g | %.3g |" % (c["rows"], c["c0"], c["c1"], r["grad_w1"], r["dbeta0"], r["dgamma0"],
                                                                         r["grad_w0_t"], r["two"]))
    lines += ["", "Worst over the %d cases: grad_w1 %.3g, dbeta0 %.3g, dgamma0 %.3g, grad_w0_t %.3g (two-pass entry: %.3g)." % (
        len(CASES), worst["grad_w1"], worst["dbeta0"], worst["dgamma0"], worst["grad_w0_t"], worst["two"])]
    return "\n".join(lines)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the package, as tests/conftest.py does under pytest
    print(render())
