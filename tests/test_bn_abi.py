"""Kernel-level parity of csrc/mlp.hip through the C ABI against plain fp64 torch formulas: every kernel and template instantiation
(the case table, the restated dispatch rule, the references and the bounds are in tests/bn_cases.py), ctypes on _lib.lib() with no
Python routing in between.

Two input families, as in tests/test_gemm_abi.py.  EXACT: small integers, integer means and power-of-two invstd, so that every sum is
an integer (or a dyadic fraction) below 2^24 and the fp32 result equals fp64 bit for bit: a dropped tail row, a row visited twice or a
wrong last block shows at any size.  ROUND: seeded normals, every element within c u M of fp64 (derived in bn_cases.py; the hardware
exponential of the ELU on load is the only measured constant).  Backward ReLU pre-activations are kept 1e-3 from zero in the rounding
family (asserted on the reference); the exact family holds pre-activations of exactly 0 on purpose.
Every output is a slice of a sentinel-filled buffer, checked after the call; strided outputs keep the sentinel in their gap columns,
strided inputs hold NaN there.  Every case runs twice and must give the same bits (fixed-order reductions)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_cases as bc  # noqa: E402
from abi_harness import RATIOS, Arena, abi, call, parity_report, place, same, twice, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = bc.EPS
U = bc.U
ELU_SEEN = {}


parity_report = parity_report("BN_PARITY_OUT", ("hf_bn", "hf_narrow_linear_dx", "mean/std"), elu=ELU_SEEN)        # the source of profiles/bn_parity.md


def workspace(a, rows, c):
    _, L = abi()
    nbytes = L.hf_bn_workspace(rows, c)
    assert nbytes == 4 * 2 * c * bc.BN_MAX_BLOCKS
    return a.out((nbytes // 4,)), nbytes


def is_exact(c):
    return c["family"] == "exact"


def momentum(c):
    return 0.25 if is_exact(c) else 0.1


def pow2(n):
    return n & (n - 1) == 0


def running_init(d, c, ch):
    if is_exact(c):
        return d.ints((ch,), -8, 8) / 4, d.ints((ch,), 0, 8) / 4
    return d.normal((ch,)), d.uniform((ch,), 0.5, 1.5)


# ------------------------------------------------------------------------------------------------------- statistics, forward
def check_statistics(c, name, x, elu, small, got, t, mom, rows=None, ch=None):
    """save_mean / save_invstd / running estimates against bn_cases.ref_stats.  Exact family: bit for bit (fp64 formula rounded once;
    running = (1 - m) r + m float(batch) with m = 1/4 and quarter-integer r is exact in fp64 and rounded once)"""
    rows, ch = rows or c["rows"], ch or c["c"]
    chain = bc.sum_chain(rows, ch, small)
    mean, var, invstd, d_mean, d_var, d_invstd = bc.ref_stats(x, elu, chain, EPS, is_exact(c))
    if is_exact(c):
        same(got["mean"], mean, name + ".save_mean")
        same(got["invstd"], invstd, name + ".save_invstd")
        if got.get("rm") is not None:
            same(got["rm"], (1 - mom) * t["rm"].double() + mom * mean.float().double(), name + ".running_mean")
            same(got["rv"], (1 - mom) * t["rv"].double() + mom * var.float().double(), name + ".running_var")
        return
    fam = c["family"]
    within(got["mean"], mean, d_mean, name + ".save_mean", fam)
    within(got["invstd"], invstd, d_invstd, name + ".save_invstd", fam)
    if got.get("rm") is not None:
        want, b = bc.running_bounds(t["rm"], mean, d_mean, mom)
        within(got["rm"], want, b, name + ".running_mean", fam)
        want, b = bc.running_bounds(t["rv"], var, d_var, mom)
        within(got["rv"], want, b, name + ".running_var", fam)


def stats_inputs(c):
    d = bc.Draw(c, DEV)
    t = dict(x=bc.make_x(d, c["rows"], c["c"], is_exact(c), False))
    t["rm"], t["rv"] = running_init(d, c, c["c"])
    return t


def run_stats(c, t, mom=None):
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, ch = c["rows"], c["c"]
    a = Arena(DEV)
    x = place(DEV, t["x"])
    mean, invstd, rm, rv = a.out((ch,)), a.out((ch,)), a.out((ch,), init=t["rm"]), a.out((ch,), init=t["rv"])
    ws, nbytes = workspace(a, rows, ch)
    call(L.hf_bn_stats(rows, ch, ptr(x), EPS, momentum(c) if mom is None else mom, ptr(rm), ptr(rv), ptr(mean), ptr(invstd), ptr(ws), nbytes, sp), "hf_bn_stats")
    a.check()
    return dict(mean=mean, invstd=invstd, rm=rm, rv=rv)


@pytest.mark.parametrize("c", bc.cases_of("stats"), ids=bc.case_id)
def test_bn_stats(c):
    """rounding family: a second call with momentum = 1 returns the batch variance itself in running_var ((1 - 1) r + 1 var): it must lie
    within the one-pass envelope c u E[x^2] of the fp64 variance, the mean/std = 30 channel (column 1) included"""
    t = stats_inputs(c)
    got = twice(run_stats, c, t)
    check_statistics(c, "hf_bn_stats", t["x"], False, False, got, t, momentum(c))
    if not is_exact(c):
        var_got = run_stats(c, t, mom=1.0)["rv"]
        chain = bc.sum_chain(c["rows"], c["c"])
        _, var, _, _, _, _ = bc.ref_stats(t["x"], False, chain, EPS, False)
        env = bc.one_pass_envelope(t["x"], False, chain) + U * var
        within(var_got, var, env, "hf_bn_stats.variance (one-pass envelope)", c["family"])
        if c["c"] > 1 and c["rows"] >= 300:
            err = float((var_got[1].double() - var[1]).abs())
            print("mean/std = 30 channel: relative variance error %.3g, share of the envelope %.3g" % (err / float(var[1]), err / float(env[1])))
            for key, v in (("mean/std = 30 channel: relative variance error", err / float(var[1])), ("mean/std = 30 channel: share of c u E[x^2]", err / float(env[1]))):
                RATIOS[(key, "round")] = max(RATIOS.get((key, "round"), 0.0), v)


def train_inputs(c):
    d = bc.Draw(c, DEV)
    ch = c["c"]
    t = dict(x=bc.make_x(d, c["rows"], ch, is_exact(c), bool(c["relu"] & 2)))
    t["gamma"], t["beta"] = bc.affine(d, ch, is_exact(c))
    t["rm"], t["rv"] = running_init(d, c, ch)
    return t


def run_train(c, t):
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, ch, ld = c["rows"], c["c"], c["ld"]
    a = Arena(DEV)
    x, gamma, beta = place(DEV, t["x"]), place(DEV, t["gamma"]), place(DEV, t["beta"])
    y = a.out((rows, ch), ld=ld)
    mean, invstd, rm, rv = a.out((ch,)), a.out((ch,)), a.out((ch,), init=t["rm"]), a.out((ch,), init=t["rv"])
    ws, nbytes = workspace(a, rows, ch)
    if ld:
        call(L.hf_bn_relu_fwd_train_ld(rows, ch, ptr(x), ptr(gamma), ptr(beta), EPS, momentum(c), ptr(rm), ptr(rv), c["relu"], ptr(y), ld, ptr(mean), ptr(invstd),
                                       ptr(ws), nbytes, sp), "hf_bn_relu_fwd_train_ld")
    else:
        call(L.hf_bn_relu_fwd_train(rows, ch, ptr(x), ptr(gamma), ptr(beta), EPS, momentum(c), ptr(rm), ptr(rv), c["relu"], ptr(y), ptr(mean), ptr(invstd),
                                    ptr(ws), nbytes, sp), "hf_bn_relu_fwd_train")
    a.check()
    return dict(y=y, mean=mean, invstd=invstd, rm=rm, rv=rv)


@pytest.mark.parametrize("c", bc.cases_of("train"), ids=bc.case_id)
def test_bn_relu_fwd_train(c):
    """statistics against fp64; y against fp64 evaluated with the statistics the kernel returned (they are what the apply pass read)"""
    t = train_inputs(c)
    got = twice(run_train, c, t)
    name = "hf_bn_relu_fwd_train" + ("_ld" if c["ld"] else "")
    small = bc.small_geom(c["rows"], c["c"]) is not None
    check_statistics(c, name, t["x"], bool(c["relu"] & 2), small, got, t, momentum(c))
    y, bound = bc.ref_apply(t["x"], t["gamma"], t["beta"], got["mean"], got["invstd"], c["relu"])
    within(got["y"], y, bound, name + ".y", c["family"])


def eval_inputs(c):
    d = bc.Draw(c, DEV)
    t = dict(x=bc.make_x(d, c["rows"], c["c"], is_exact(c), bool(c["relu"] & 2)))
    t["bn"] = bc.given_stats(d, c["c"], is_exact(c))
    return t


def run_eval(c, t):
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, ch = c["rows"], c["c"]
    a = Arena(DEV)
    x = place(DEV, t["x"])
    bn = [place(DEV, v) for v in t["bn"]]
    y = a.out((rows, ch))
    call(L.hf_bn_relu_fwd_eval(rows, ch, ptr(x), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), c["relu"], ptr(y), sp), "hf_bn_relu_fwd_eval")
    a.check()
    return dict(y=y)


@pytest.mark.parametrize("c", bc.cases_of("eval"), ids=bc.case_id)
def test_bn_relu_fwd_eval(c):
    t = eval_inputs(c)
    got = twice(run_eval, c, t)
    y, bound = bc.ref_apply(t["x"], *t["bn"], c["relu"])
    if is_exact(c):
        same(got["y"], y, "hf_bn_relu_fwd_eval.y")
    else:
        within(got["y"], y, bound, "hf_bn_relu_fwd_eval.y", c["family"])


# ------------------------------------------------------------------------------------------------------- backward
def bwd_inputs(c):
    d = bc.Draw(c, DEV)
    rows, ch, relu = c["rows"], c["c"], c["relu"]
    t = dict(x=bc.make_x(d, rows, ch, is_exact(c), bool(relu & 2)), bn=bc.given_stats(d, ch, is_exact(c)))
    t["dy"] = d.ints((rows, ch), -2, 2) if is_exact(c) else d.normal((rows, ch))
    if not is_exact(c) and relu & 1:
        bc.nudge(t["x"], *t["bn"], relu)
        assert bc.margin(t["x"], *t["bn"], relu) >= bc.RELU_MARGIN
    if c["kind"] == "bwd_dx":
        if is_exact(c):
            k = rows if pow2(rows) else 0
            t["dgamma"], t["dbeta"] = d.ints((ch,), -1, 1) * k, d.ints((ch,), -1, 1) * k
        else:
            t["dgamma"], t["dbeta"] = d.normal((ch,)) * rows ** 0.5, d.normal((ch,)) * rows ** 0.5
    return t


def run_bwd(c, t):
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, ch, ld = c["rows"], c["c"], c["ld"]
    a = Arena(DEV)
    x, dy = place(DEV, t["x"]), place(DEV, t["dy"], ld=ld)
    bn = [place(DEV, v) for v in t["bn"]]
    dx, dgamma, dbeta = a.out((rows, ch)), a.out((ch,)), a.out((ch,))
    colsum = a.out((ch,)) if c["colsum"] else None
    ws, nbytes = workspace(a, rows, ch)
    if ld:
        call(L.hf_bn_relu_bwd_ld(rows, ch, ptr(x), ptr(dy), ld, ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), c["relu"], ptr(dx), ptr(dgamma), ptr(dbeta),
                                 ptr(colsum), ptr(ws), nbytes, sp), "hf_bn_relu_bwd_ld")
    else:
        call(L.hf_bn_relu_bwd(rows, ch, ptr(x), ptr(dy), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), c["relu"], ptr(dx), ptr(dgamma), ptr(dbeta),
                              ptr(colsum), ptr(ws), nbytes, sp), "hf_bn_relu_bwd")
    a.check()
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, colsum=colsum)


def check_backward(c, name, r, got, rows, chain_dx, exact_dx):
    """dbeta / dgamma against fp64; dx against fp64 evaluated with the sums the kernel returned (its dx pass read those); the column
    sums against the fp64 sum of the dx it stored"""
    fam = c["family"]
    if is_exact(c) and r["m"] == 0:
        same(got["dbeta"], r["dbeta"], name + ".dbeta")
        same(got["dgamma"], r["dgamma"], name + ".dgamma")
    else:
        within(got["dbeta"], r["dbeta"], r["d_dbeta"], name + ".dbeta", fam)
        within(got["dgamma"], r["dgamma"], r["d_dgamma"], name + ".dgamma", fam)
    dx, bound = bc.ref_bn_dx(r, got["dgamma"], got["dbeta"], rows)
    if exact_dx:
        same(got["dx"], dx, name + ".dx")
    else:
        within(got["dx"], dx, bound, name + ".dx", fam)
    if got.get("colsum") is not None:
        s, b = bc.ref_colsum(got["dx"], chain_dx)
        within(got["colsum"], s, b, name + ".dx_colsum", fam)


@pytest.mark.parametrize("c", bc.cases_of("bwd"), ids=bc.case_id)
def test_bn_relu_bwd(c):
    t = bwd_inputs(c)
    got = twice(run_bwd, c, t)
    small = bc.small_geom(c["rows"], c["c"]) is not None
    chain = bc.sum_chain(c["rows"], c["c"], small)
    r = bc.ref_bn_bwd(t["x"], t["dy"], *t["bn"], c["relu"], chain)
    check_backward(c, "hf_bn_relu_bwd" + ("_ld" if c["ld"] else ""), r, got, c["rows"], chain, is_exact(c) and pow2(c["rows"]))


def run_bwd_dx(c, t):
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, ch = c["rows"], c["c"]
    a = Arena(DEV)
    x, dy, dgamma, dbeta = place(DEV, t["x"]), place(DEV, t["dy"]), place(DEV, t["dgamma"]), place(DEV, t["dbeta"])
    bn = [place(DEV, v) for v in t["bn"]]
    dx = a.out((rows, ch))
    call(L.hf_bn_relu_bwd_dx(rows, ch, ptr(x), ptr(dy), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), ptr(dgamma), ptr(dbeta), c["relu"], ptr(dx), sp),
         "hf_bn_relu_bwd_dx")
    a.check()
    return dict(dx=dx)


@pytest.mark.parametrize("c", bc.cases_of("bwd_dx"), ids=bc.case_id)
def test_bn_relu_bwd_dx(c):
    t = bwd_inputs(c)
    got = twice(run_bwd_dx, c, t)
    r = bc.ref_bn_bwd(t["x"], t["dy"], *t["bn"], c["relu"], 1)
    dx, bound = bc.ref_bn_dx(r, t["dgamma"], t["dbeta"], c["rows"])
    if is_exact(c):
        same(got["dx"], dx, "hf_bn_relu_bwd_dx.dx")
    else:
        within(got["dx"], dx, bound, "hf_bn_relu_bwd_dx.dx", c["family"])


# ------------------------------------------------------------------------------------------------------- fused dropout
STATE0 = 0x0123456789abcdef
CALLS_BEFORE = 5


def drop_inputs(c):
    """forward: even channels gamma = 0, beta = 2 in the exact family (y there IS the mask: 2 scale or 0), the others a plain affine;
    backward: statistics as inputs, as bwd_inputs"""
    d = bc.Draw(c, DEV)
    rows, ch, relu = c["rows"], c["c"], c["relu"]
    t = bwd_inputs(dict(c, kind="bwd"))
    t["gamma"], t["beta"] = bc.affine(d, ch, is_exact(c))
    if is_exact(c):
        t["gamma"][0::2], t["beta"][0::2] = 0.0, 2.0
    t["rm"], t["rv"] = running_init(d, c, ch)
    return t


def _i64(v):
    return v - (1 << 64) if v >= (1 << 63) else v


def run_drop(c, t):
    """two consecutive forward calls on one layer state, then the backward pass with the seed the second call returned"""
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, ch, relu, rate, salt = c["rows"], c["c"], c["relu"], c["rate"], c["salt"]
    a = Arena(DEV)
    x, gamma, beta, dy = place(DEV, t["x"]), place(DEV, t["gamma"]), place(DEV, t["beta"]), place(DEV, t["dy"])
    bn = [place(DEV, v) for v in t["bn"]]
    state = torch.tensor([_i64(STATE0 + ch), CALLS_BEFORE], dtype=torch.int64, device=DEV)
    out = {}
    for n in (1, 2):
        y, mean, invstd = a.out((rows, ch)), a.out((ch,)), a.out((ch,))
        seed = torch.zeros(1, dtype=torch.int64, device=DEV)
        ws, nbytes = workspace(a, rows, ch)
        call(L.hf_bn_dropout_fwd_train(rows, ch, ptr(x), ptr(gamma), ptr(beta), EPS, momentum(c), None, None, relu, rate, salt, ptr(state), ptr(seed), ptr(y),
                                       ptr(mean), ptr(invstd), ptr(ws), nbytes, sp), "hf_bn_dropout_fwd_train")
        out.update({"y%d" % n: y, "seed%d" % n: seed, "mean": mean, "invstd": invstd})
    dx, dgamma, dbeta = a.out((rows, ch)), a.out((ch,)), a.out((ch,))
    ws, nbytes = workspace(a, rows, ch)
    call(L.hf_bn_dropout_bwd(rows, ch, ptr(x), ptr(dy), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), relu, rate, ptr(out["seed2"]), ptr(dx), ptr(dgamma),
                             ptr(dbeta), ptr(ws), nbytes, sp), "hf_bn_dropout_bwd")
    a.check()
    out.update(dx=dx, dgamma=dgamma, dbeta=dbeta, state=state)
    return out


@pytest.mark.parametrize("c", bc.cases_of("drop"), ids=bc.case_id)
def test_bn_dropout(c):
    """the seeds, the call counter and the mask against the integer restatement of bn_cases.py (independent of the kernel: the mask is
    never read back from the code under test); forward values and the backward pass against fp64 under the restated mask"""
    t = drop_inputs(c)
    got = twice(run_drop, c, t)
    rows, ch, relu = c["rows"], c["c"], c["relu"]
    thresh, scale = bc.drop_threshold(c["rate"])
    if c["rate"] == 0.0:
        assert thresh == 0 and scale == 1.0
    if c["rate"] >= 0.99999:
        assert thresh == 65535
    state = [int(v) & bc.M64 for v in got["state"].tolist()]
    assert state == [(STATE0 + ch) & bc.M64, CALLS_BEFORE + 2], "drop_state: base seed unchanged, call counter advanced by one per call"
    seeds = [bc.drop_seed(STATE0 + ch, c["salt"], CALLS_BEFORE + n) for n in (1, 2)]
    assert [int(got["seed%d" % n].item()) & bc.M64 for n in (1, 2)] == seeds
    small = False
    check_statistics(c, "hf_bn_dropout_fwd_train", t["x"], bool(relu & 2), small, got, t, momentum(c))
    keeps = [torch.from_numpy(bc.drop_keep(rows, ch, s, thresh)).to(DEV) for s in seeds]
    if 0.0 < c["rate"] < 0.9:
        assert not torch.equal(keeps[0], keeps[1]), "two calls draw two masks"
    for n, keep in zip((1, 2), keeps):
        y = got["y%d" % n]
        assert bool((y[~keep] == 0).all()), "a dropped element is not zero"
        if is_exact(c):         # the mask, element for element, in the channels whose pre-dropout value is exactly 2
            want = keep[:, 0::2].double() * 2.0 * float(scale)
            same(y[:, 0::2], want, "hf_bn_dropout_fwd_train.y (mask)")
        mult = keep.double() * float(scale)
        ref, bound = bc.ref_apply(t["x"], t["gamma"], t["beta"], got["mean"], got["invstd"], relu, mult, 2)
        within(y, ref, bound, "hf_bn_dropout_fwd_train.y", c["family"])
    mult = keeps[1].double() * float(scale)
    chain = bc.sum_chain(rows, ch)
    r = bc.ref_bn_bwd(t["x"], t["dy"], *t["bn"], relu, chain, mult, 2)
    if is_exact(c) and float(scale) in (1.0, 2.0):
        r["m"] = 0              # a power-of-two scale: dh = dy scale is exact
    check_backward(c, "hf_bn_dropout_bwd", r, got, rows, chain, False)
    zero = (t["bn"][0] == 0)
    assert bool((got["dx"][:, zero] == 0).all())


# ------------------------------------------------------------------------------------------------------- BN + ReLU + max-pool
def first_argmax(h):
    """(groups, k, c) -> (max, its FIRST row): the rule of the kernel"""
    hmax = h.max(dim=1).values
    k = h.shape[1]
    idx = torch.where(h == hmax[:, None, :], torch.arange(k, device=h.device)[None, :, None], k).min(dim=1).values
    return hmax, idx


def pool_inputs(c):
    d = bc.Draw(c, DEV)
    g, k, ch = c["groups"], c["k"], c["c"]
    # rounding family: on a grid of 1 / 512, so that two rows of a column are either equal (a tie: the first wins) or 2e-3 apart -- the
    # reference's top two then differ by far more than the forward bound, or not at all (asserted in pool_reference)
    z = (d.ints((g, k, ch), -2, 2) if is_exact(c) else torch.round(d.normal((g, k, ch), 0.3, 1.0) * 512) / 512)
    if k > 1:
        z[0::3, k // 2:, :] = z[0::3, :1, :]            # a third of the groups: tail rows repeat the first row (padded neighbourhoods)
    t = dict(z=z.reshape(g * k, ch), bn=bc.given_stats(d, ch, is_exact(c)))
    t["gamma"], t["beta"] = bc.affine(d, ch, is_exact(c))
    t["dp"] = d.ints((g, ch), -2, 2) if is_exact(c) else d.normal((g, ch))
    t["rm"], t["rv"] = running_init(d, c, ch)
    if not is_exact(c):
        bc.nudge(t["z"], *t["bn"], 1)
        if k > 1:
            zz = t["z"].view(g, k, ch)
            zz[0::3, k // 2:, :] = zz[0::3, :1, :]
        assert bc.margin(t["z"], *t["bn"], 1) >= bc.RELU_MARGIN
    return t


def pool_reference(c, z, gamma, beta, mean, invstd):
    """pooled, its bound and the arg-max; asserts that the arg-max is decided: every row within twice the bound of the maximum is a copy
    of the winning row (then the first one wins in the kernel too), and an all-clamped column has no pre-activation near zero"""
    g, k, ch = c["groups"], c["k"], c["c"]
    h, bound = bc.ref_apply(z, gamma, beta, mean, invstd, 1)
    h, bound, z3 = h.view(g, k, ch), bound.view(g, k, ch), z.view(g, k, ch)
    hmax, idx = first_argmax(h)
    bmax = bound.max(dim=1).values
    if not is_exact(c):
        pre = bc.pre_activation(z, gamma, beta, mean, invstd, 1).view(g, k, ch)
        zwin = torch.gather(z3, 1, idx[:, None, :])
        rival = (h >= hmax[:, None, :] - 2 * bmax[:, None, :]) & (z3 != zwin) & (hmax[:, None, :] > 0)
        assert not bool(rival.any()), "the reference's top two are closer than the forward bound"
        assert not bool(((hmax == 0)[:, None, :] & (pre > -2 * bound)).any())
    return hmax, bmax, idx


def run_pool(c, t):
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    g, k, ch, tr = c["groups"], c["k"], c["c"], c["training"]
    a = Arena(DEV)
    z, dp = place(DEV, t["z"]), place(DEV, t["dp"])
    bn = [place(DEV, v) for v in t["bn"]]
    gamma, beta = (place(DEV, t["gamma"]), place(DEV, t["beta"])) if tr else (bn[0], bn[1])
    pooled, argmax = a.out((g, ch)), a.out((g, ch), dtype=torch.uint8)
    ws, nbytes = workspace(a, g * k, ch)
    if tr:
        mean, invstd, rm, rv = a.out((ch,)), a.out((ch,)), a.out((ch,), init=t["rm"]), a.out((ch,), init=t["rv"])
    else:
        mean, invstd, rm, rv = bn[2], bn[3], None, None
    call(L.hf_bn_relu_maxpool_fwd(g, k, ch, ptr(z), ptr(gamma), ptr(beta), tr, EPS, momentum(c), ptr(rm), ptr(rv), ptr(mean), ptr(invstd), ptr(pooled), ptr(argmax),
                                  ptr(ws), nbytes, sp), "hf_bn_relu_maxpool_fwd")
    a.check()
    # backward: the statistics are plain inputs; it runs on the given ones and on the reference's arg-max under them
    _, _, idx = pool_reference(c, t["z"], *t["bn"])
    am = place(DEV, idx.to(torch.uint8))
    dz, dgamma, dbeta = a.out((g * k, ch)), a.out((ch,)), a.out((ch,))
    colsum = a.out((ch,)) if c["colsum"] else None
    ws2, nbytes = workspace(a, g * k, ch)
    call(L.hf_bn_relu_maxpool_bwd(g, k, ch, ptr(z), ptr(dp), ptr(am), ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), ptr(dz), ptr(dgamma), ptr(dbeta), ptr(colsum),
                                  ptr(ws2), nbytes, sp), "hf_bn_relu_maxpool_bwd")
    a.check()
    return dict(pooled=pooled, argmax=argmax, mean=mean if tr else None, invstd=invstd if tr else None, rm=rm, rv=rv, dx=dz, dgamma=dgamma, dbeta=dbeta,
                colsum=colsum)


@pytest.mark.parametrize("c", bc.cases_of("pool"), ids=bc.case_id)
def test_bn_relu_maxpool(c):
    t = pool_inputs(c)
    got = twice(run_pool, c, t)
    g, k, ch, fam = c["groups"], c["k"], c["c"], c["family"]
    rows = g * k
    if c["training"]:
        check_statistics(c, "hf_bn_relu_maxpool_fwd", t["z"], False, False, got, t, momentum(c), rows, ch)
        used = (t["gamma"], t["beta"], got["mean"], got["invstd"])
    else:
        used = t["bn"]
    hmax, bmax, idx = pool_reference(c, t["z"], *used)
    if is_exact(c) and not c["training"]:
        same(got["pooled"], hmax, "hf_bn_relu_maxpool_fwd.pooled")
    else:
        within(got["pooled"], hmax, bmax, "hf_bn_relu_maxpool_fwd.pooled", fam)
    assert torch.equal(got["argmax"].long(), idx), "arg-max: the first maximum wins"
    # backward under the given statistics: dh is dpooled at the arg-max row where the ReLU is open
    _, _, idx_b = pool_reference(c, t["z"], *t["bn"])
    onehot = torch.zeros(g, k, ch, dtype=torch.float64, device=DEV).scatter_(1, idx_b[:, None, :], t["dp"].double()[:, None, :])
    r = bc.ref_bn_bwd(t["z"], onehot.view(rows, ch), *t["bn"], 1, bc.sum_chain(g, ch))
    check_backward(c, "hf_bn_relu_maxpool_bwd", r, got, rows, bc.sum_chain(rows, ch), is_exact(c) and pow2(rows))


# ------------------------------------------------------------------------------------------------------- narrow linear
def narrow_inputs(c):
    d = bc.Draw(c, DEV)
    if is_exact(c):
        return dict(g=d.ints((c["rows"], c["cout"]), -2, 2), w=d.ints((c["cout"], c["cin"]), -2, 2))
    return dict(g=d.normal((c["rows"], c["cout"])), w=d.normal((c["cout"], c["cin"]), 0.0, 0.5))


def run_narrow(c, t):
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    a = Arena(DEV)
    g, w = place(DEV, t["g"]), place(DEV, t["w"])
    dx = a.out((c["rows"], c["cin"]))
    call(L.hf_narrow_linear_dx(c["rows"], c["cin"], c["cout"], ptr(g), ptr(w), ptr(dx), sp), "hf_narrow_linear_dx")
    a.check()
    return dict(dx=dx)


@pytest.mark.parametrize("c", bc.cases_of("narrow"), ids=bc.case_id)
def test_narrow_linear_dx(c):
    t = narrow_inputs(c)
    got = twice(run_narrow, c, t)
    dx, bound = bc.ref_narrow(t["g"], t["w"])
    if is_exact(c):
        same(got["dx"], dx, "hf_narrow_linear_dx.dx")
    else:
        within(got["dx"], dx, bound, "hf_narrow_linear_dx.dx", c["family"])


# ------------------------------------------------------------------------------------------------------- the measured constant
def test_elu_constant_covers_the_hardware_exponential():
    """the ELU on load alone: hf_bn_relu_fwd_eval with gamma = invstd = 1, mean = beta = 0 returns elu(x) with no other rounding.  Worst
    |got - ref64| / (u (exp(x) + 1)) over the ELU inputs of the cases (N(0.3, 1) and the mean-30 channel, the edge inputs, a dense sweep of
    [-104, 0]) must stay at or below ELU_C / 2: ELU_C is the next power of two at or above twice the measured ELU_MEASURED"""
    c = bc._case("eval", rows=33000, c=64, relu=2, family="round")
    d = bc.Draw(c, DEV)
    x = bc.make_x(d, 33000, 64, False, True)
    x[:, 3] = torch.linspace(-104.0, 0.0, 33000, device=DEV)
    x[:, 4] = -torch.logspace(-9, 0, 33000, device=DEV)
    t = dict(x=x, bn=(torch.ones(64, device=DEV), torch.zeros(64, device=DEV), torch.zeros(64, device=DEV), torch.ones(64, device=DEV)))
    got = run_eval(c, t)["y"]
    neg = x <= 0
    ref = torch.expm1(x.double())
    diff = (got.double() - ref).abs()[neg]
    ratio = float((diff / (U * (torch.exp(x.double()) + 1.0))[neg]).max())
    rel = float((diff / (U * ref.abs()[neg]).clamp(min=1e-300)).max())
    print("ELU on load: worst |got - ref64| / (u (exp(x) + 1)) = %.4g; relative to u |ref| = %.4g" % (ratio, rel))
    ELU_SEEN.update(ratio=ratio, relative_to_ref=rel)
    assert torch.equal(got[~neg], x[~neg])
    assert 2 * ratio <= bc.ELU_C
    assert bc.ELU_C == 2.0 ** int(np.ceil(np.log2(2 * bc.ELU_MEASURED))) and ratio <= 1.001 * bc.ELU_MEASURED


# ------------------------------------------------------------------------------------------------------- argument checks
def test_bad_arguments_are_rejected_before_anything_is_launched():
    """completes test_mlp_entry_points_reject_bad_arguments: every call below returns HF_EINVAL (HF_EWORKSPACE for the short
    workspace) and leaves every output buffer at the sentinel"""
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    EINVAL, EWS = _lib.HF_EINVAL, _lib.HF_EWORKSPACE
    rows, ch = 64, 8
    a = Arena(DEV)
    x = place(DEV, torch.ones(rows, ch))
    xo = place(DEV, torch.ones(rows, ch), off=True)
    v = place(DEV, torch.ones(ch))
    y, yo, wide = a.out((rows, ch)), a.out((rows, ch), off=True), a.out((rows, ch), ld=ch + 2)
    o1, o2, o3 = a.out((ch,)), a.out((ch,)), a.out((ch,))
    am = a.out((rows, ch), dtype=torch.uint8)
    state = a.out((2,), dtype=torch.int64)
    seed = a.out((1,), dtype=torch.int64)
    ws, n = workspace(a, rows, ch)
    P = ptr
    train = lambda x_, y_, n_=n: L.hf_bn_relu_fwd_train(rows, ch, P(x_), P(v), P(v), EPS, 0.1, None, None, 1, P(y_), P(o1), P(o2), P(ws), n_, sp)
    train_ld = lambda ld: L.hf_bn_relu_fwd_train_ld(rows, ch, P(x), P(v), P(v), EPS, 0.1, None, None, 1, P(wide), ld, P(o1), P(o2), P(ws), n, sp)
    bwd = lambda x_, dy_, dx_, n_=n: L.hf_bn_relu_bwd(rows, ch, P(x_), P(dy_), P(v), P(v), P(v), P(v), 1, P(dx_), P(o1), P(o2), P(o3), P(ws), n_, sp)
    bwd_ld = lambda ld: L.hf_bn_relu_bwd_ld(rows, ch, P(x), P(x), ld, P(v), P(v), P(v), P(v), 1, P(y), P(o1), P(o2), None, P(ws), n, sp)
    drop = lambda rate, n_=n: L.hf_bn_dropout_fwd_train(rows, ch, P(x), P(v), P(v), EPS, 0.1, None, None, 1, rate, 0, P(state), P(seed), P(y), P(o1), P(o2), P(ws),
                                                        n_, sp)
    drop_bwd = lambda rate: L.hf_bn_dropout_bwd(rows, ch, P(x), P(x), P(v), P(v), P(v), P(v), 1, rate, P(seed), P(y), P(o1), P(o2), P(ws), n, sp)
    pool = lambda k, z_=x, n_=n: L.hf_bn_relu_maxpool_fwd(rows // 4, k, ch, P(z_), P(v), P(v), 1, EPS, 0.1, None, None, P(o1), P(o2), P(y), P(am), P(ws), n_, sp)
    pool_bwd = lambda k, dz_=y, n_=n: L.hf_bn_relu_maxpool_bwd(rows // 4, k, ch, P(x), P(x), P(am), P(v), P(v), P(v), P(v), P(dz_), P(o1), P(o2), None, P(ws), n_,
                                                                  sp)
    bad = {
        "x one float off a 16-byte boundary, c % 4 == 0": (train(xo, y), EINVAL),
        "y off": (train(x, yo), EINVAL),
        "eval: x off": (L.hf_bn_relu_fwd_eval(rows, ch, P(xo), P(v), P(v), P(v), P(v), 1, P(y), sp), EINVAL),
        "eval: y off": (L.hf_bn_relu_fwd_eval(rows, ch, P(x), P(v), P(v), P(v), P(v), 1, P(yo), sp), EINVAL),
        "stats: x off": (L.hf_bn_stats(rows, ch, P(xo), EPS, 0.1, None, None, P(o1), P(o2), P(ws), n, sp), EINVAL),
        "bwd: x off": (bwd(xo, x, y), EINVAL), "bwd: dy off": (bwd(x, xo, y), EINVAL), "bwd: dx off": (bwd(x, x, yo), EINVAL),
        "bwd_dx: dx off": (L.hf_bn_relu_bwd_dx(rows, ch, P(x), P(x), P(v), P(v), P(v), P(v), P(v), P(v), 1, P(yo), sp), EINVAL),
        "narrow: dx off": (L.hf_narrow_linear_dx(rows, ch, 2, P(x), P(x), P(yo), sp), EINVAL),
        "pool: z off": (pool(4, xo), EINVAL), "pool backward: dz off": (pool_bwd(4, yo), EINVAL),
        "ldy < c": (train_ld(ch - 1), EINVAL), "lddy < c": (bwd_ld(ch - 1), EINVAL),
        "ldy % 4 != 0 with 16-byte accesses": (train_ld(ch + 2), EINVAL), "lddy % 4 != 0": (bwd_ld(ch + 2), EINVAL),
        "k = 256": (pool(256), EINVAL), "k = 256 backward": (pool_bwd(256), EINVAL), "k = 0": (pool(0), EINVAL),
        "cout = 5": (L.hf_narrow_linear_dx(rows, ch, 5, P(x), P(x), P(y), sp), EINVAL),
        "cout = 0": (L.hf_narrow_linear_dx(rows, ch, 0, P(x), P(x), P(y), sp), EINVAL),
        "rate = 1": (drop(1.0), EINVAL), "rate < 0": (drop(-0.25), EINVAL), "rate = nan": (drop(float("nan")), EINVAL), "backward rate = 1": (drop_bwd(1.0), EINVAL),
        "short workspace": (train(x, y, n - 1), EWS), "short workspace: bwd": (bwd(x, x, y, n - 1), EWS), "short workspace: dropout": (drop(0.5, n - 1), EWS),
        "short workspace: pool": (pool(4, x, n - 1), EWS), "short workspace: pool backward": (pool_bwd(4, y, n - 1), EWS),
        "short workspace: stats": (L.hf_bn_stats(rows, ch, P(x), EPS, 0.1, None, None, P(o1), P(o2), P(ws), n - 1, sp), EWS),
        "rows = 0": (L.hf_bn_relu_fwd_eval(0, ch, P(x), P(v), P(v), P(v), P(v), 1, P(y), sp), EINVAL),
    }
    wrong = {k: got for k, (got, want) in bad.items() if got != want}
    assert not wrong, wrong
    a.untouched()


def test_channel_limits_are_rejected_before_anything_is_launched():
    """include/hfops.h: c <= 4096, and c <= 1024 where c % 4 != 0 (a workgroup then has c threads per row).  One past each limit is
    HF_EINVAL with every output untouched; the limit itself is served (1023: the widest scalar-width row; 4096) and checked against fp64 by
    the cases (1500, 1023) and (7, 4096) / (12803, 4096) above"""
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    EINVAL = _lib.HF_EINVAL
    rows = 8
    for ch, want in ((1023, 0), (1024, 0), (1025, EINVAL), (2047, EINVAL), (4095, EINVAL), (4096, 0), (4097, EINVAL), (4100, EINVAL)):
        assert bc.launch_limit_ok(ch) == (want == 0)
        a = Arena(DEV)
        x = place(DEV, torch.ones(rows, ch))
        v, z0 = place(DEV, torch.ones(ch)), place(DEV, torch.zeros(ch))
        g4 = place(DEV, torch.ones(rows, 4))
        y, o1, o2, o3 = a.out((rows, ch)), a.out((ch,)), a.out((ch,)), a.out((ch,))
        pooled, am = a.out((rows // 4, ch)), a.out((rows // 4, ch), dtype=torch.uint8)
        am0, dp = place(DEV, torch.zeros(rows // 4, ch, dtype=torch.uint8)), place(DEV, torch.ones(rows // 4, ch))
        state, seed = a.out((2,), dtype=torch.int64), a.out((1,), dtype=torch.int64)
        n = 4 * 2 * ch * bc.BN_MAX_BLOCKS
        ws = a.out((n // 4,))
        P = ptr
        status = {
            "hf_bn_stats": L.hf_bn_stats(rows, ch, P(x), EPS, 0.1, None, None, P(o1), P(o2), P(ws), n, sp),
            "hf_bn_relu_fwd_train": L.hf_bn_relu_fwd_train(rows, ch, P(x), P(v), P(v), EPS, 0.1, None, None, 1, P(y), P(o1), P(o2), P(ws), n, sp),
            "hf_bn_relu_fwd_train_ld": L.hf_bn_relu_fwd_train_ld(rows, ch, P(x), P(v), P(v), EPS, 0.1, None, None, 1, P(y), ch, P(o1), P(o2), P(ws), n, sp),
            "hf_bn_relu_fwd_eval": L.hf_bn_relu_fwd_eval(rows, ch, P(x), P(v), P(v), P(z0), P(v), 1, P(y), sp),
            "hf_bn_relu_bwd": L.hf_bn_relu_bwd(rows, ch, P(x), P(x), P(v), P(v), P(z0), P(v), 1, P(y), P(o1), P(o2), P(o3), P(ws), n, sp),
            "hf_bn_relu_bwd_ld": L.hf_bn_relu_bwd_ld(rows, ch, P(x), P(x), ch, P(v), P(v), P(z0), P(v), 1, P(y), P(o1), P(o2), P(o3), P(ws), n, sp),
            "hf_bn_relu_bwd_dx": L.hf_bn_relu_bwd_dx(rows, ch, P(x), P(x), P(v), P(v), P(z0), P(v), P(z0), P(z0), 1, P(y), sp),
            "hf_bn_dropout_fwd_train": L.hf_bn_dropout_fwd_train(rows, ch, P(x), P(v), P(v), EPS, 0.1, None, None, 1, 0.5, 0, P(state), P(seed), P(y), P(o1), P(o2),
                                                                 P(ws), n, sp),
            "hf_bn_dropout_bwd": L.hf_bn_dropout_bwd(rows, ch, P(x), P(x), P(v), P(v), P(z0), P(v), 1, 0.5, P(seed), P(y), P(o1), P(o2), P(ws), n, sp),
            "hf_bn_relu_maxpool_fwd": L.hf_bn_relu_maxpool_fwd(rows // 4, 4, ch, P(x), P(v), P(v), 1, EPS, 0.1, None, None, P(o1), P(o2), P(pooled), P(am), P(ws), n,
                                                               sp),
            "hf_bn_relu_maxpool_bwd": L.hf_bn_relu_maxpool_bwd(rows // 4, 4, ch, P(x), P(dp), P(am0), P(v), P(v), P(z0), P(v), P(y), P(o1), P(o2), P(o3), P(ws),
                                                               n, sp),
            "hf_narrow_linear_dx": L.hf_narrow_linear_dx(rows, ch, 4, P(g4), P(x), P(y), sp),
        }
        wrong = {k: s for k, s in status.items() if s != want}
        assert not wrong, (ch, wrong)
        if want:
            a.untouched()
        else:
            a.check()
            assert bool(torch.isfinite(y).all())


def render_parity(report):
    """profiles/bn_parity.md from the JSON that a session with BN_PARITY_OUT wrote"""
    lines = ["# Parity of csrc/mlp.hip with fp64 through the C ABI", "",
             "Worst `|got - ref64| / bound` of every output over the cases of `tests/bn_cases.py`, one MI355X session of",
             "`BN_PARITY_OUT=report.json pytest -m gpu tests/test_bn_abi.py`; rendered by `python tests/test_bn_abi.py report.json`.",
             "The bounds are the derived `c u M` of `tests/bn_cases.py`; outputs of the exact family that are compared bit for bit do not appear",
             "(their tolerance is zero).  Every ratio must be <= 1; those >= 0.5 are marked.", "",
             "| output | family | worst ratio | |", "|---|---|---:|---|"]
    notes = []
    for key, v in sorted(report["ratios"].items()):
        name, fam = key.split("|")
        if name.startswith("mean/std"):
            notes.append("- %s: %.3g" % (name, v))
            continue
        lines.append("| `%s` | %s | %.3g | %s |" % (name, fam, v, "**>= 0.5**" if v >= 0.5 else ""))
    lines += ["", "One-pass variance, the mean/std = 30 channel of the `hf_bn_stats` rounding cases (worst over the cases):"] + notes
    lines += ["", "ELU on load (`hf_bn_relu_fwd_eval`, gamma = invstd = 1, mean = beta = 0, 2.1 M inputs): worst `|got - ref64| / (u (exp(x) + 1))` = %.4g"
              % report["elu"]["ratio"], "(`ELU_MEASURED`; `ELU_C` = %g is the next power of two at or above twice that).  Relative to `u |ref|` the same error is %.3g:"
              % (bc.ELU_C, report["elu"]["relative_to_ref"]), "the subtraction in `exp(x) - 1` cancels near 0, which is why the bound is on the magnitude sum of the two terms."]
    return "\n".join(lines)


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        print(render_parity(json.load(f)))
