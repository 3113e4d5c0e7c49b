"""Kernel-level parity of csrc/gemm.hip through the C ABI against plain fp64 torch formulas: every template instantiation (the case
table and the references are in tests/gemm_cases.py), no Python routing predicate between the test and the kernel.

Two input families.  EXACT: small-integer operands and integer-valued BatchNorm affines, so every product and partial sum is an
integer below 2^24 and the fp32 result must equal the fp64 reference bit for bit, whatever the summation order -- dropped or doubled
rows, wrong tile edges and stale prefetches show at any size.  ROUND: seeded normal inputs with non-trivial constants, every element
within c * u * M of the fp64 reference (c and M derived in the docstrings of gemm_cases.py; tolerance zero everywhere else).  ReLU
pre-activations are kept 1e-3 away from zero (asserted), so no mask can flip and no element is left out of any comparison.
Every output is a slice of a larger buffer filled with a sentinel: the floats before and after it must be unchanged after the call."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402
from abi_harness import Arena, abi, call, place, same, within  # noqa: E402
from gemm_runs import UNSET, lift_inputs, run_lift_bwd  # noqa: E402,F401  (test_gemm_cases_cpu.py replaces run_lift_bwd here)

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, MOMENTUM = 1e-3, 0.1
TWO24 = float(2 ** 24)


# ------------------------------------------------------------------------------------------------------- forward
def fwd_inputs(c):
    g = gc.generator(c)
    rows, cin, cout, exact = c["rows"], c["cin"], c["cout"], c["family"] == "exact"
    t = {}
    if exact:
        nonneg = c["elu"]                       # ELU is the identity on non-negative pre-activations
        t["x"] = gc.ints(g, (rows, cin), 0 if nonneg else -2, 2)
        t["w"] = gc.ints(g, (cout, cin), 0, 2) if nonneg else (gc.sparse_pm1(g, (cout, cin)) if rows > 100000 else gc.ints(g, (cout, cin), -2, 2))
        t["bias"] = gc.ints(g, (cout,), -2, 2) if c["bias"] else None
        t["bn"] = gc.bn_consts(g, cin, True, nonneg) if c["act"] else None
    else:
        t["x"] = torch.randn(rows, cin, generator=g) + 0.3
        t["w"] = torch.randn(cout, cin, generator=g) * 0.5
        t["bias"] = torch.randn(cout, generator=g) if c["bias"] else None
        t["bn"] = gc.bn_consts(g, cin, False) if c["act"] else None
        if c["act"] and not c["elu"]:
            assert gc.nudge_share_ok(gc.nudge_off_relu_threshold(t["x"], *t["bn"]), t["x"].numel())
    if c["act"] and not c["elu"] and not exact:
        assert gc.relu_margin(t["x"], *t["bn"]) >= gc.RELU_MARGIN
    t["rm"], t["rv"] = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5
    return t


def run_fwd(c, t):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, cin, cout, mis = c["rows"], c["cin"], c["cout"], c["misalign"]
    a = Arena(DEV)
    x, w = place(DEV, t["x"], mis == "x"), place(DEV, t["w"], mis == "weight")
    bias = place(DEV, t["bias"])
    bn = [place(DEV, v) for v in t["bn"]] if t["bn"] else [None] * 4
    z, mean, invstd = a.out((rows, cout)), a.out((cout,)), a.out((cout,))
    xact = a.out((rows, cin), off=mis == "x_act") if c["xact"] else None
    rm = a.out((cout,), init=t["rm"]) if c["running"] in (1, 2) else None
    rv = a.out((cout,), init=t["rv"]) if c["running"] in (1, 3) else None
    nbytes = L.hf_linear_bn_fwd_workspace(cout)
    ws = a.out((nbytes // 4,))
    if c["elu"]:
        call(L.hf_linear_elu_bn_fwd(rows, cin, cout, ptr(x), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), ptr(xact), ptr(w), ptr(z), EPS, MOMENTUM,
                                    ptr(rm), ptr(rv), ptr(mean), ptr(invstd), ptr(ws), nbytes, sp), "hf_linear_elu_bn_fwd")
    else:
        call(L.hf_linear_bn_fwd(rows, cin, cout, ptr(x), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), ptr(xact), ptr(w), ptr(bias), ptr(z), EPS,
                                MOMENTUM, ptr(rm), ptr(rv), ptr(mean), ptr(invstd), ptr(ws), nbytes, sp), "hf_linear_bn_fwd")
    a.check()
    return dict(z=z, x_act=xact, mean=mean, invstd=invstd, rm=rm, rv=rv)


def check_statistics(c, got, ref, s64, nt):
    """mean / invstd / running estimates.  Exact family with every per-workgroup sum an integer below 2^24: the sums are exact, the
    division and the variance are fp64, what is left is the cast of the result (1 rounding; 2 for invstd: var + eps was cast from
    float).  Otherwise the derived bounds of gemm_cases.stats_bounds."""
    rows = c["rows"]
    d_mean, d_var, d_invstd = ref["d_mean"], ref["d_var"], ref["d_invstd"]
    if c["family"] == "exact" and gc.tiles_per_workgroup(rows, nt) * gc.FWD_ROWS * float(s64.abs().max()) ** 2 < TWO24 and bool((s64 == s64.round()).all()):
        d_mean, d_var, d_invstd = gc.U * ref["mean"].abs(), gc.U * ref["var"], 2 * gc.U * ref["invstd"]
    within(got["mean"], ref["mean"], d_mean, "mean")
    within(got["invstd"], ref["invstd"], d_invstd, "invstd")
    return d_mean, d_var


def check_running(got, t, ref, d_mean, d_var, flag, m0="rm", v0="rv"):
    if flag in (1, 2):
        want, b = gc.running_bounds(t[m0].to(DEV), ref["mean"], d_mean, MOMENTUM)
        within(got["rm"], want, b, "running_mean")
    if flag in (1, 3):
        want, b = gc.running_bounds(t[v0].to(DEV), ref["var"], d_var, MOMENTUM)
        within(got["rv"], want, b, "running_var")


def check_fwd(c, t, got):
    rows, cout = c["rows"], c["cout"]
    nt = gc.cdiv(cout, 32)
    dv = lambda v: None if v is None else v.to(DEV)
    bn = [dv(v) for v in t["bn"]] if t["bn"] else None
    ref = gc.ref_linear_fwd(dv(t["x"]), bn, dv(t["w"]), dv(t["bias"]), c["elu"], 16 * gc.tiles_per_workgroup(rows, nt) + 4, EPS)
    if c["family"] == "exact":
        same(got["z"], ref["z"], "z")
        if c["xact"]:
            same(got["x_act"], ref["h"], "x_act")
    else:
        within(got["z"], ref["z"], ref["z_err"], "z")
        if c["xact"]:
            within(got["x_act"], ref["h"], ref["h_err"], "x_act")
    s64 = gc.elu64(ref["z"]) if c["elu"] else ref["z"]
    d_mean, d_var = check_statistics(c, got, ref, s64, nt)
    check_running(got, t, ref, d_mean, d_var, c["running"])


@pytest.mark.parametrize("c", gc.sweep_cases("fwd"), ids=gc.case_id)
def test_linear_bn_fwd(c):
    t = fwd_inputs(c)
    check_fwd(c, t, run_fwd(c, t))


# ------------------------------------------------------------------------------------------------------- input gradient
def bwd_inputs(c):
    g = gc.generator(c)
    rows, cout, cin, form, exact = c["rows"], c["cout"], c["cin"], c["form"], c["family"] == "exact"
    from_dy, sums = form.startswith("dy"), form.endswith("sums")
    t = dict(z=None, bn=None, dgamma=None, dbeta=None, zprev=None, pbn=None)
    if exact:
        t["dy"], t["wt"] = gc.ints(g, (rows, cout), -2, 2), gc.ints(g, (cin, cout), -2, 2)
        if from_dy:
            t["z"], t["bn"] = gc.ints(g, (rows, cout), -2, 2), gc.bn_consts(g, cout, True)
            t["dgamma"], t["dbeta"] = torch.zeros(cout), torch.zeros(cout)
        if sums:
            t["zprev"], t["pbn"] = gc.ints(g, (rows, cin), 0 if c["elu"] else -2, 2), gc.bn_consts(g, cin, True)
    else:
        t["dy"], t["wt"] = torch.randn(rows, cout, generator=g), torch.randn(cin, cout, generator=g) * 0.5
        if from_dy:
            t["z"], t["bn"] = torch.randn(rows, cout, generator=g) + 0.3, gc.bn_consts(g, cout, False)
            t["dgamma"], t["dbeta"] = torch.randn(cout, generator=g) * rows ** 0.5, torch.randn(cout, generator=g) * rows ** 0.5
            assert gc.nudge_share_ok(gc.nudge_off_relu_threshold(t["z"], *t["bn"]), t["z"].numel())
            assert gc.relu_margin(t["z"], *t["bn"]) >= gc.RELU_MARGIN
        if sums:
            t["zprev"], t["pbn"] = torch.randn(rows, cin, generator=g) + 0.3, gc.bn_consts(g, cin, False)
            if not c["elu"]:
                assert gc.nudge_share_ok(gc.nudge_off_relu_threshold(t["zprev"], *t["pbn"]), t["zprev"].numel())
                assert gc.relu_margin(t["zprev"], *t["pbn"]) >= gc.RELU_MARGIN
    return t


def run_bwd(c, t):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, cout, cin, form, mis = c["rows"], c["cout"], c["cin"], c["form"], c["misalign"]
    from_dy, sums = form.startswith("dy"), form.endswith("sums")
    a = Arena(DEV)
    dy, wt, z = place(DEV, t["dy"], mis == "dy"), place(DEV, t["wt"], mis == "weight_t"), place(DEV, t["z"], mis == "z")
    bn = [place(DEV, v) for v in t["bn"]] if t["bn"] else [None] * 4
    pbn = [place(DEV, v) for v in t["pbn"]] if t["pbn"] else [None] * 4
    dgamma, dbeta, zprev = place(DEV, t["dgamma"]), place(DEV, t["dbeta"]), place(DEV, t["zprev"])
    dx = a.out((rows, cin)) if "dx" in form else None
    dz_out = a.out((rows, cout), off=mis == "dz_out") if from_dy else None
    pdg, pdb = (a.out((cin,)), a.out((cin,))) if sums else (None, None)
    nbytes = L.hf_linear_bn_bwd_workspace(cin)
    ws = a.out((nbytes // 4,))
    if c["elu"]:
        call(L.hf_linear_elu_bn_bwd(rows, cout, cin, ptr(dy), ptr(wt), ptr(dx), ptr(zprev), ptr(pbn[0]), ptr(pbn[1]), ptr(pbn[2]), ptr(pbn[3]), ptr(pdg),
                                    ptr(pdb), ptr(ws), nbytes, sp), "hf_linear_elu_bn_bwd")
    else:
        call(L.hf_linear_bn_bwd(rows, cout, cin, ptr(dy), ptr(z), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), ptr(dgamma), ptr(dbeta), ptr(dz_out),
                                ptr(wt), ptr(dx), ptr(zprev), ptr(pbn[0]), ptr(pbn[1]), ptr(pbn[2]), ptr(pbn[3]), ptr(pdg), ptr(pdb), ptr(ws), nbytes,
                                sp), "hf_linear_bn_bwd")
    a.check()
    return dict(dx=dx, dz_out=dz_out, p_dgamma=pdg, p_dbeta=pdb)


def check_bwd(c, t, got):
    dv = lambda v: None if v is None else v.to(DEV)
    nt = gc.cdiv(c["cin"], 32)
    ref = gc.ref_linear_bwd(dv(t["dy"]), dv(t["z"]), [dv(v) for v in t["bn"]] if t["bn"] else None, dv(t["dgamma"]), dv(t["dbeta"]), dv(t["wt"]),
                            dv(t["zprev"]), [dv(v) for v in t["pbn"]] if t["pbn"] else None, c["elu"],
                            16 * gc.tiles_per_workgroup(c["rows"], nt) + 4)
    exact = c["family"] == "exact"
    for name, key in (("dx", "dx"), ("dz_out", "dz")):
        if got[name] is not None:
            if exact:
                same(got[name], ref[key], name)
            else:
                within(got[name], ref[key], ref[key + "_err"], name)
    if got["p_dbeta"] is not None:
        if exact and float(ref["sum_abs"].max()) < TWO24:      # integer sums below 2^24: no rounding anywhere
            same(got["p_dbeta"], ref["p_dbeta"], "p_dbeta")
            same(got["p_dgamma"], ref["p_dgamma"], "p_dgamma")
        else:
            within(got["p_dbeta"], ref["p_dbeta"], ref["d_p_dbeta"], "p_dbeta")
            within(got["p_dgamma"], ref["p_dgamma"], ref["d_p_dgamma"], "p_dgamma")


@pytest.mark.parametrize("c", gc.sweep_cases("bwd"), ids=gc.case_id)
def test_linear_bn_bwd(c):
    t = bwd_inputs(c)
    check_bwd(c, t, run_bwd(c, t))


# ------------------------------------------------------------------------------------------------------- weight gradient
def wgrad_inputs(c):
    g = gc.generator(c)
    rows, cout, cin, exact = c["rows"], c["cout"], c["cin"], c["family"] == "exact"
    if exact:
        t = dict(g=gc.ints(g, (rows, cout), -2, 2), x=gc.ints(g, (rows, cin), -2, 2), bn=gc.bn_consts(g, cin, True) if c["act"] else None)
    else:
        t = dict(g=torch.randn(rows, cout, generator=g), x=torch.randn(rows, cin, generator=g) + 0.3,
                 bn=gc.bn_consts(g, cin, False) if c["act"] else None)
        if c["act"]:
            assert gc.nudge_share_ok(gc.nudge_off_relu_threshold(t["x"], *t["bn"]), t["x"].numel())
            assert gc.relu_margin(t["x"], *t["bn"]) >= gc.RELU_MARGIN
    return t


def run_wgrad(c, t, short_by=0):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, cout, cin, mis = c["rows"], c["cout"], c["cin"], c["misalign"]
    a = Arena(DEV)
    gz, x = place(DEV, t["g"], mis == "grad_z"), place(DEV, t["x"], mis == "x")
    bn = [place(DEV, v) for v in t["bn"]] if t["bn"] else [None] * 4
    dw = a.out((cout, cin))
    nbytes = L.hf_linear_wgrad_workspace(rows, cout, cin)
    assert nbytes == 4 * gc.wgrad_plan(rows, cout, cin)[3] * cout * cin
    ws = a.out((nbytes // 4,))          # exactly the bytes the library asks for, guarded like an output
    status = L.hf_linear_wgrad(rows, cout, cin, ptr(gz), ptr(x), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), ptr(dw), ptr(ws), nbytes - short_by, sp)
    if short_by:
        return status
    call(status, "hf_linear_wgrad")
    a.check()
    return dict(dw=dw)


def check_wgrad(c, t, got, operand=None):
    dv = lambda v: None if v is None else v.to(DEV)
    x = dv(t["x"]) if operand is None else operand
    _, _, rpc, chunks = gc.wgrad_plan(c["rows"], c["cout"], x.shape[1])
    ref = gc.ref_wgrad(dv(t["g"]), x, [dv(v) for v in t["bn"]] if t.get("bn") else None, rpc, chunks)
    if c["family"] == "exact":
        same(got["dw"], ref["dw"], "dW")
    else:
        within(got["dw"], ref["dw"], ref["dw_err"], "dW")


@pytest.mark.parametrize("c", gc.sweep_cases("wgrad"), ids=gc.case_id)
def test_linear_wgrad(c):
    t = wgrad_inputs(c)
    check_wgrad(c, t, run_wgrad(c, t))


# ------------------------------------------------------------------------------------------------------- gather forms
def gather_inputs(c):
    """integers (the gather forms are exact-family only: the rounding behaviour is the dense kernel's); family "round": normal numbers, for the
    determinism test"""
    g = gc.generator(c)
    b, rpc, n_src, cf, cout = c["clouds"], c["rows_per_cloud"], c["n_src"], c["c_feat"], c["cout"]
    rows, cin = b * rpc, (cf + 3) // 4 * 4 + 4
    draw = (lambda shape: gc.ints(g, shape, -2, 2)) if c["family"] == "exact" else (lambda shape: torch.randn(shape, generator=g))
    return dict(points=draw((b, n_src, cf)) if cf else None, idx=torch.randint(0, n_src, (rows,), generator=g, dtype=torch.int32),
                gxyz=draw((rows, 3)), w=draw((cout, cin)), bias=draw((cout,)) if c.get("bias") else None, g=draw((rows, cout)), rows=rows, cin=cin)


def run_gather_fwd(c, t):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, cout, mis = t["rows"], c["cout"], c["misalign"]
    a = Arena(DEV)
    points, idx, gxyz = place(DEV, t["points"], mis == "points"), place(DEV, t["idx"]), place(DEV, t["gxyz"])
    w, bias = place(DEV, t["w"], mis == "weight"), place(DEV, t["bias"])
    z, mean, invstd = a.out((rows, cout)), a.out((cout,)), a.out((cout,))
    nbytes = L.hf_linear_bn_fwd_workspace(cout)
    ws = a.out((nbytes // 4,))
    call(L.hf_linear_bn_fwd_gather(rows, c["c_feat"], cout, ptr(points), c["n_src"], c["rows_per_cloud"], ptr(idx), ptr(gxyz), ptr(w), ptr(bias), ptr(z),
                                   EPS, MOMENTUM, None, None, ptr(mean), ptr(invstd), ptr(ws), nbytes, sp), "hf_linear_bn_fwd_gather")
    a.check()
    return dict(z=z, mean=mean, invstd=invstd)


def run_gather_wgrad(c, t):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, cout, cin, mis = t["rows"], c["cout"], t["cin"], c["misalign"]
    a = Arena(DEV)
    points, idx, gxyz, gz = place(DEV, t["points"], mis == "points"), place(DEV, t["idx"]), place(DEV, t["gxyz"]), place(DEV, t["g"], mis == "grad_z")
    dw = a.out((cout, cin))
    nbytes = L.hf_linear_wgrad_workspace(rows, cout, cin)
    ws = a.out((nbytes // 4,))
    call(L.hf_linear_wgrad_gather(rows, cout, c["c_feat"], ptr(gz), ptr(points), c["n_src"], c["rows_per_cloud"], ptr(idx), ptr(gxyz), ptr(dw), ptr(ws),
                                  nbytes, sp), "hf_linear_wgrad_gather")
    a.check()
    return dict(dw=dw)


def gathered(c, t):
    dv = lambda v: None if v is None else v.to(DEV)
    return gc.gather_operand(dv(t["points"]), dv(t["idx"]), dv(t["gxyz"]), c["rows_per_cloud"])


@pytest.mark.parametrize("c", gc.sweep_cases("gather_fwd"), ids=gc.case_id)
def test_linear_bn_fwd_gather(c):
    """reference: the dense formula on the materialised [features | 0-pad | x y z 0] operand"""
    t = gather_inputs(c)
    got = run_gather_fwd(c, t)
    dense = dict(c, rows=t["rows"], cin=t["cin"], elu=False, xact=False, running=0)
    ref = gc.ref_linear_fwd(gathered(c, t), None, t["w"].to(DEV), None if t["bias"] is None else t["bias"].to(DEV), False,
                            16 * gc.tiles_per_workgroup(t["rows"], gc.cdiv(c["cout"], 32)) + 4, EPS)
    same(got["z"], ref["z"], "z")
    check_statistics(dense, got, ref, ref["z"], gc.cdiv(c["cout"], 32))


@pytest.mark.parametrize("c", gc.sweep_cases("gather_wgrad"), ids=gc.case_id)
def test_linear_wgrad_gather(c):
    t = gather_inputs(c)
    check_wgrad(dict(c, rows=t["rows"]), t, run_gather_wgrad(c, t), operand=gathered(c, t))


# ------------------------------------------------------------------------------------------------------- lifting family
def run_lift_eval(c, t, w1_off=False):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, c0, c1 = c["rows"], c["c0"], c["c1"]
    a = Arena(DEV)
    x3, w0, w1 = place(DEV, t["x3"]), place(DEV, t["w0"]), place(DEV, t["w1"], w1_off)
    bn0, bn1 = [place(DEV, v) for v in t["bn0"]], [place(DEV, v) for v in t["bn1"]]
    out = a.out((rows, c1))
    nbytes = L.hf_lift_elu_bn_fwd_workspace(c0, c1)
    ws = a.out((nbytes // 4,))
    if c["kind"] == "lift_eval":
        status = L.hf_lift_elu_fwd_eval(rows, c0, c1, ptr(x3), ptr(w0), ptr(bn0[0]), ptr(bn0[1]), ptr(bn0[2]), ptr(bn0[3]), ptr(w1), ptr(out), ptr(ws), nbytes, sp)
    else:
        status = L.hf_lift_elu_fwd_eval_bn(rows, c0, c1, ptr(x3), ptr(w0), ptr(bn0[0]), ptr(bn0[1]), ptr(bn0[2]), ptr(bn0[3]), ptr(w1), ptr(bn1[0]),
                                           ptr(bn1[1]), ptr(bn1[2]), ptr(bn1[3]), ptr(out), ptr(ws), nbytes, sp)
    if w1_off:
        return status
    call(status, "hf_" + c["kind"])
    a.check()
    return dict(out=out)


@pytest.mark.parametrize("c", gc.sweep_cases("lift_eval", "lift_eval_bn"), ids=gc.case_id)
def test_lift_elu_fwd_eval(c):
    """given statistics: the exact family, bit for bit"""
    t = lift_inputs(c)
    got = run_lift_eval(c, t)
    dv = lambda v: v.to(DEV)
    _, e0, _, _ = gc.ref_lift_first(dv(t["x3"]), dv(t["w0"]))
    ref = gc.ref_lift_second(e0, torch.zeros_like(e0), [dv(v) for v in t["bn0"]], dv(t["w1"]), [dv(v) for v in t["bn1"]], 1, EPS)
    assert float(ref["y0"].min()) >= 0
    if c["kind"] == "lift_eval":
        same(got["out"], ref["z1"], "z1")
    else:
        assert float(ref["z1"].min()) >= 0
        same(got["out"], ref["y1"], "y1")


def run_lift_train(c, t):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, c0, c1 = c["rows"], c["c0"], c["c1"]
    a = Arena(DEV)
    x3, w0, w1, g0, b0 = place(DEV, t["x3"]), place(DEV, t["w0"]), place(DEV, t["w1"]), place(DEV, t["bn0"][0]), place(DEV, t["bn0"][1])
    z1 = a.out((rows, c1))
    mean0, invstd0, mean1, invstd1 = a.out((c0,)), a.out((c0,)), a.out((c1,)), a.out((c1,))
    rm0, rv0, rm1, rv1 = a.out((c0,), init=t["rm0"]), a.out((c0,), init=t["rv0"]), a.out((c1,), init=t["rm1"]), a.out((c1,), init=t["rv1"])
    nbytes = L.hf_lift_elu_bn_fwd_workspace(c0, c1)
    ws = a.out((nbytes // 4,))
    call(L.hf_lift_elu_bn_fwd(rows, c0, c1, ptr(x3), ptr(w0), ptr(g0), ptr(b0), EPS, MOMENTUM, ptr(rm0), ptr(rv0), ptr(mean0), ptr(invstd0), ptr(w1),
                              ptr(z1), EPS, MOMENTUM, ptr(rm1), ptr(rv1), ptr(mean1), ptr(invstd1), ptr(ws), nbytes, sp), "hf_lift_elu_bn_fwd")
    a.check()
    return dict(z1=z1, mean0=mean0, invstd0=invstd0, mean1=mean1, invstd1=invstd1, rm0=rm0, rv0=rv0, rm1=rm1, rv1=rv1)


def check_lift_train(c, t, got):
    """the first layer's statistics against fp64; the second GEMM against fp64 evaluated with the constants it was given, i.e. the
    fp32 mean0 / invstd0 the first half produced (they are its inputs); then the second layer's statistics"""
    dv = lambda v: v.to(DEV)
    rows = c["rows"]
    _, e0, e_err, _ = gc.ref_lift_first(dv(t["x3"]), dv(t["w0"]))
    mean, var, invstd, d_mean, d_var, d_invstd = gc.stats_bounds(e0, e_err, gc.lift_stats_chain(rows), EPS)
    within(got["mean0"], mean, d_mean, "mean0")
    within(got["invstd0"], invstd, d_invstd, "invstd0")
    first = dict(mean=mean, var=var)
    check_running(dict(rm=got["rm0"], rv=got["rv0"]), t, first, d_mean, d_var, 1, "rm0", "rv0")
    bn0 = [dv(t["bn0"][0]), dv(t["bn0"][1]), got["mean0"], got["invstd0"]]
    ref = gc.ref_lift_second(e0, e_err, bn0, dv(t["w1"]), None, 16 * gc.tiles_per_workgroup(rows, gc.cdiv(c["c1"], 32)) + 4, EPS)
    within(got["z1"], ref["z1"], ref["z1_err"], "z1")
    within(got["mean1"], ref["mean"], ref["d_mean"], "mean1")
    within(got["invstd1"], ref["invstd"], ref["d_invstd"], "invstd1")
    check_running(dict(rm=got["rm1"], rv=got["rv1"]), t, ref, ref["d_mean"], ref["d_var"], 1, "rm1", "rv1")


@pytest.mark.parametrize("c", gc.sweep_cases("lift_train"), ids=gc.case_id)
def test_lift_elu_bn_fwd(c):
    t = lift_inputs(c)
    check_lift_train(c, t, run_lift_train(c, t))


@pytest.mark.parametrize("c", gc.sweep_cases("lift_bwd"), ids=gc.case_id)
def test_lift_elu_bn_bwd(c):
    """against fp64 autograd of z1 = BN0_batch(elu(x3 W0^T)) W1^T; the kernel is given the reference's batch statistics rounded to
    fp32 (bounds: gemm_cases.lift_bwd_bounds)"""
    t = lift_inputs(c)
    dv = lambda v: v.to(DEV)
    rows, c0, c1 = c["rows"], c["c0"], c["c1"]
    gw1, gg0, gb0, gw0, mean, invstd = gc.ref_lift_bwd_autograd(dv(t["x3"]), dv(t["w0"]), dv(t["bn0"][0]), dv(t["bn0"][1]), dv(t["w1"]), dv(t["dz1"]), EPS)
    got = run_lift_bwd(c, t, (mean.float(), invstd.float()))
    _, _, rpc, chunks = gc.wgrad_plan(rows, c1, c0)
    b = gc.lift_bwd_bounds(dv(t["x3"]), dv(t["w0"]), [dv(t["bn0"][0]), dv(t["bn0"][1]), mean, invstd], dv(t["w1"]), dv(t["dz1"]),
                           16 * gc.tiles_per_workgroup(rows, gc.cdiv(c0, 32)) + 4, min(rows, rpc) + gc.cdiv(chunks, 16) + 15)
    within(got["grad_w1"], gw1, b["d_w1"], "grad_w1")
    within(got["dbeta0"], gb0, b["d_dbeta"], "dbeta0")
    within(got["dgamma0"], gg0, b["d_dgamma"], "dgamma0")
    within(got["grad_w0_t"], gw0.t(), b["d_w0"].t(), "grad_w0_t")


# ------------------------------------------------------------------------------------------------------- alignment, determinism, limits
# tests/test_gemm_cases_cpu.py replaces the run_* functions of this module (by these names) with fp32 torch evaluations on the host
RUNNERS = dict(fwd=(fwd_inputs, run_fwd), bwd=(bwd_inputs, run_bwd), wgrad=(wgrad_inputs, run_wgrad), gather_fwd=(gather_inputs, run_gather_fwd),
               gather_wgrad=(gather_inputs, run_gather_wgrad))


def _run(c):
    if c["kind"] == "lift_bwd":
        t = lift_inputs(c)
        return run_lift_bwd(c, t, (t["bn0"][2], t["bn0"][3]))
    if c["kind"] == "lift_train":
        return run_lift_train(c, lift_inputs(c))
    if c["kind"] in ("lift_eval", "lift_eval_bn"):
        return run_lift_eval(c, lift_inputs(c))
    make, run = RUNNERS[c["kind"]]
    return run(c, make(c))


@pytest.mark.parametrize("c", gc.ALIGN_CASES, ids=gc.case_id)
def test_operand_one_float_off_a_16_byte_boundary(c):
    """channel counts stay multiples of 4, one pointer that the launcher's alignment test inspects is offset by one float: the scalar
    twin of the kernel runs, same arithmetic order, so every output is bit-identical to the aligned call"""
    assert gc.instantiations(c) != gc.instantiations(dict(c, misalign=None)) or c["kind"] in ("lift_bwd", "gather_fwd", "gather_wgrad")
    off, aligned = _run(c), _run(dict(c, misalign=None))
    for k in aligned:
        if aligned[k] is not None:
            assert torch.equal(off[k], aligned[k]), k


DETERMINISM_CASES = [
    gc._case("fwd", elu=False, rows=40013, cin=100, cout=161, act=True, xact=True, bias=True, running=1, family="round"),
    gc._case("fwd", elu=True, rows=40013, cin=33, cout=225, act=True, xact=True, bias=False, running=1, family="round"),
    gc._case("bwd", rows=40013, cout=64, cin=161, form="dy_dx_dzout", elu=False, family="round"),
    gc._case("bwd", rows=40013, cout=64, cin=225, form="dz_dx_sums", elu=False, family="round"),
    gc._case("bwd", rows=40013, cout=33, cin=100, form="dz_dx_sums", elu=True, family="round"),
    gc._case("wgrad", rows=200003, cout=129, cin=65, act=True, family="round"),
    gc._case("gather_fwd", clouds=3, rows_per_cloud=5000, n_src=170, c_feat=5, cout=100, bias=True, family="round"),
    gc._case("gather_wgrad", clouds=3, rows_per_cloud=5000, n_src=170, c_feat=64, cout=65, family="round"),
    gc._case("lift_train", rows=40000, c0=36, c1=100, family="round"),
    gc._case("lift_eval", rows=40000, c0=164, c1=100, family="round"),
    gc._case("lift_eval_bn", rows=40000, c0=36, c1=225, family="round"),
    gc._case("lift_bwd", rows=40000, c0=96, c1=100, family="round"),
]


@pytest.mark.parametrize("c", DETERMINISM_CASES, ids=gc.case_id)
def test_two_calls_give_the_same_bits(c):
    """the header promises fixed-order reductions (no atomics)"""
    first, second = _run(c), _run(c)
    for k in first:
        if first[k] is not None:
            assert torch.equal(first[k], second[k]), k


def test_limits_are_rejected_before_anything_is_launched():
    """completes test_mlp_entry_points_reject_bad_arguments: one past each documented limit of include/hfops.h is HF_EINVAL, the limit
    itself is accepted by the same call"""
    _lib, L = abi(UNSET)
    sp = _lib.stream_ptr()
    EINVAL, EWS = _lib.HF_EINVAL, _lib.HF_EWORKSPACE
    buf = torch.zeros(32 * 16384, device=DEV)
    buf[8 * 16384:9 * 16384] = 1.0                                          # q(8): a vector of ones (invstd)
    q = lambda i: _lib.ptr(buf[i * 16384:])                                 # disjoint 64 KiB regions, each at a 16-byte boundary
    off = lambda i: _lib.ptr(buf[i * 16384 + 1:])
    wsb, wbuf = torch.zeros(1 << 22, device=DEV), torch.zeros(1024 * 384, device=DEV)
    wp = _lib.ptr(wbuf)                                                     # the largest weight of the calls below
    ws, n = _lib.ptr(wsb), wsb.numel() * 4
    rows = 8
    fwd = lambda cin, cout: L.hf_linear_bn_fwd(rows, cin, cout, q(0), None, None, None, None, None, wp, None, q(2), EPS, MOMENTUM, None, None, q(3), q(4), ws,
                                               n, sp)
    elu_fwd = lambda cin, cout: L.hf_linear_elu_bn_fwd(rows, cin, cout, q(0), None, None, None, None, None, wp, q(2), EPS, MOMENTUM, None, None, q(3), q(4),
                                                       ws, n, sp)
    for f in (fwd, elu_fwd):
        assert [f(32, 257), f(1025, 32), f(1024, 256)] == [EINVAL, EINVAL, 0]
    bwd = lambda cout, cin, z: L.hf_linear_bn_bwd(rows, cout, cin, q(0), z, q(8), q(5), q(5), q(8), q(5), q(5), None, wp, q(2), None, None, None, None, None,
                                                  None, None, ws, n, sp)
    assert [bwd(32, 257, None), bwd(257, 32, q(3)), bwd(256, 256, q(3)), bwd(384, 256, None)] == [EINVAL, EINVAL, 0, 0]
    elu_bwd = lambda cin: L.hf_linear_elu_bn_bwd(rows, 32, cin, q(0), q(1), q(2), q(3), q(8), q(5), q(5), q(8), q(6), q(7), ws, n, sp)
    assert [elu_bwd(257), elu_bwd(256)] == [EINVAL, 0]
    for c0, w1, want in ((6, q(1), EINVAL), (260, q(1), EINVAL), (36, off(1), EINVAL), (256, q(1), 0)):
        assert L.hf_lift_elu_bn_fwd(rows, c0, 32, q(0), q(9), q(8), q(5), EPS, MOMENTUM, None, None, q(3), q(4), w1, q(2), EPS, MOMENTUM, None, None, q(6), q(7),
                                    ws, n, sp) == want
        assert L.hf_lift_elu_fwd_eval(rows, c0, 32, q(0), q(9), q(8), q(5), q(5), q(8), w1, q(2), ws, n, sp) == want
        assert L.hf_lift_elu_fwd_eval_bn(rows, c0, 32, q(0), q(9), q(8), q(5), q(5), q(8), w1, q(8), q(5), q(5), q(8), q(2), ws, n, sp) == want
    for c0, want in ((6, EINVAL), (164, EINVAL), (160, 0)):
        assert L.hf_lift_elu_bn_bwd(rows, c0, 32, q(0), q(9), q(8), q(5), q(5), q(8), q(10), q(1), q(11), q(12), q(13), q(14), ws, n, sp) == want
    torch.cuda.synchronize()
    c = gc._case("wgrad", rows=257, cout=65, cin=33, act=False)
    assert run_wgrad(c, wgrad_inputs(c), short_by=1) == EWS
