"""The fused X-Conv backward through the C ABI and its comparison with the fp64 references of tests/xconv_cases.py, as a plain module:
what more than one of tests/test_xconv_abi.py, test_xconv_bwd_diet_abi.py, test_xconv_bwd_fw_abi.py and test_xconv_bn_abi.py needs."""
import ctypes

import numpy as np

import xconv_cases as xc
from abi_harness import SENTINEL, Arena, In, Out, abi, call, dev64, same, within

DEV = "cuda"


def compare(c, got, want, mag, n, name):
    """exact: bit for bit against fp64 rounded once; rounding: within n u M"""
    want = dev64(DEV, want).reshape(got.shape)
    if c["family"] == "exact":
        same(got, want, name)
    else:
        b = dev64(DEV, xc.bound(n, mag)).reshape(got.shape)
        within(got, want, b, name, c["family"])


def is_exact(c):
    return c["family"] == "exact"


def dense_f(c, t):
    return xc.concat_f(c, t).astype(np.float32)


BWD_SHAPES = dict(x=lambda c: xc.rows_of(c) * c["k"] * c["k"], f=lambda c: xc.rows_of(c) * c["k"] * (c["c0"] if c["gather"] else c["c0"] + c["c1"]),
                  wd=lambda c: c["k"] * (c["c0"] + c["c1"]) * c["m"], fts=lambda c: c["b"] * c["n"] * c["c1"])


def run_bwd(c, t, ws=None):
    """-> (dict of the gradients, route seen in the workspace: 'staged' / 'direct' / None)"""
    _lib, L = abi()
    sp = _lib.stream_ptr()
    rows, k, m, c0, c1 = xc.rows_of(c), c["k"], c["m"], c["c0"], c["c1"]
    ws = c["ws"] if ws is None else ws
    a = Arena(DEV)
    x, wd, go = In(DEV, t["x"]), In(DEV, t["wd"]), In(DEV, t["go"], "go" in c["off"])
    names = xc.ALL4 if c["gather"] else xc.ALL4[:3]
    g = {n: Out(a, BWD_SHAPES[n](c), passed=n in c["want"], off=(n == "fts" and "gfts" in c["off"])) for n in names}
    seen = None
    if c["gather"]:
        fd, fts, idx, off, ent = In(DEV, t["fd"]), In(DEV, t["fts"]), In(DEV, t["idx"]), In(DEV, t["offsets"]), In(DEV, t["entries"])
        nbytes = L.hf_xconv_depthwise_gather_grad_workspace(c["b"], c["p"], k, c0, c1, m) if ws else 0
        assert nbytes == (xc.gather_grad_workspace(c["b"], c["p"], k, c0, c1, m) if ws else 0), "the workspace size restated in xconv_cases.py"
        w = Out(a, nbytes // 4, passed=bool(ws and nbytes), fill=SENTINEL)
        call(L.hf_xconv_depthwise_gather_grad(c["b"], c["n"], c["p"], k, c0, c1, m, x.p, fd.p, fts.p, idx.p, wd.p, go.p, off.p, ent.p, g["x"].p, g["f"].p,
                                              g["fts"].p, g["wd"].p, w.p, nbytes, sp), "hf_xconv_depthwise_gather_grad")
        if ws and nbytes and rows:
            block = w.view[:rows * k * c1]
            kept = block == SENTINEL
            seen = "direct" if bool(kept.all()) else "staged"
            assert seen == "direct" or not bool(kept.any()), "the staging region is partly written"
    else:
        f = In(DEV, dense_f(c, t))
        call(L.hf_xconv_depthwise_grad(rows, k, c0 + c1, m, x.p, f.p, wd.p, go.p, g["x"].p, g["f"].p, g["wd"].p, sp), "hf_xconv_depthwise_grad")
    a.check()
    for n in names:
        if not g[n].passed:
            assert bool((g[n].view == SENTINEL).all()), "grad_%s was not asked for and was written" % n
    return {n: g[n].view for n in names if g[n].passed}, seen


# ------------------------------------------------------------------------------------------------------- the backward with the short grad_x path
def n_grad_x(c):
    """roundings on the longest path into one entry of grad_x, from xc_bwd_x_rows' add order"""
    n = c["m"] + xc.cdiv(c["c0"] + c["c1"], 64) + 6
    assert n <= xc.roundings(c)["x"], "grad_x: %d roundings, more than xconv_cases.roundings allows" % n
    return n


def check_bwd_short_x(c, t, got, entry):
    ref = xc.ref_fused_bwd(c, t, c["want"])
    mag = {} if is_exact(c) else xc.ref_fused_bwd(c, t, c["want"], mag=True)
    n = xc.roundings(c, t)
    n["x"] = n_grad_x(c)
    for name in got:
        compare(c, got[name], ref[name], mag.get(name), n[name], "%s.grad_%s" % (entry, name))


def folded_inputs(c):
    """the case's inputs with z1 in place of F_delta and the four BatchNorm constants"""
    t = xc.make_inputs(c)
    rng = np.random.default_rng(xc._seed(c) ^ 0x5eed)
    c0 = c["c0"]
    if is_exact(c):
        t["z1"] = rng.integers(1, 3, t["fd"].shape).astype(np.float32)
        t["gamma"], t["invstd"] = np.ones(c0, np.float32), np.ones(c0, np.float32)
        t["mean"], t["beta"] = np.zeros(c0, np.float32), np.zeros(c0, np.float32)
    else:
        t["z1"] = t["fd"]
        t["gamma"], t["invstd"] = rng.uniform(0.5, 1.5, c0).astype(np.float32), rng.uniform(0.5, 2.0, c0).astype(np.float32)
        t["mean"], t["beta"] = (0.1 * rng.standard_normal(c0)).astype(np.float32), (0.1 * rng.standard_normal(c0)).astype(np.float32)
    return t


def run_folded(c, t):
    """-> (the gradients of hf_xconv_depthwise_gather_bn_grad, those of hf_bn_relu_fwd_eval + hf_xconv_depthwise_gather_grad with a
    workspace, F_delta as the library normalises it)"""
    _lib, L = abi()
    sp = _lib.stream_ptr()
    b, n, p, k, c0, c1, m = c["b"], c["n"], c["p"], c["k"], c["c0"], c["c1"], c["m"]
    rows = b * p
    d = {name: In(DEV, t[name]) for name in ("x", "z1", "fts", "wd", "go", "gamma", "beta", "mean", "invstd", "idx", "offsets", "entries")}
    a = Arena(DEV)
    f = Out(a, rows * k * c0)
    call(L.hf_bn_relu_fwd_eval(rows * k, c0, d["z1"].p, d["gamma"].p, d["beta"].p, d["mean"].p, d["invstd"].p, 2, f.p, sp), "hf_bn_relu_fwd_eval")
    res = []
    for folded in (True, False):
        g = {name: Out(a, BWD_SHAPES[name](c), passed=name in c["want"]) for name in xc.ALL4}
        if folded:
            dg, db = Out(a, c0, passed="f" in c["want"]), Out(a, c0, passed="f" in c["want"])
            nbytes = L.hf_xconv_depthwise_gather_bn_grad_workspace(b, p, k, c0, c1, m)
            ws = Out(a, nbytes // 4, fill=SENTINEL)
            call(L.hf_xconv_depthwise_gather_bn_grad(b, n, p, k, c0, c1, m, d["x"].p, d["z1"].p, d["gamma"].p, d["beta"].p, d["mean"].p,
                                                     d["invstd"].p, d["fts"].p, d["idx"].p, d["wd"].p, d["go"].p, d["offsets"].p,
                                                     d["entries"].p, g["x"].p, g["f"].p, g["fts"].p, g["wd"].p, dg.p, db.p, ws.p, nbytes, sp),
                 "hf_xconv_depthwise_gather_bn_grad")
        else:
            nbytes = L.hf_xconv_depthwise_gather_grad_workspace(b, p, k, c0, c1, m)
            ws = Out(a, nbytes // 4, fill=SENTINEL)
            call(L.hf_xconv_depthwise_gather_grad(b, n, p, k, c0, c1, m, d["x"].p, f.p, d["fts"].p, d["idx"].p, d["wd"].p, d["go"].p,
                                                  d["offsets"].p, d["entries"].p, g["x"].p, g["f"].p, g["fts"].p, g["wd"].p, ws.p, nbytes, sp),
                 "hf_xconv_depthwise_gather_grad")
        a.check()
        for name in xc.ALL4:
            if not g[name].passed:
                assert bool((g[name].view == SENTINEL).all()), "grad_%s was not asked for and was written" % name
        res.append({name: g[name].view for name in xc.ALL4 if g[name].passed})
    return res[0], res[1], f.view


# ------------------------------------------------------------------------------------------------------- argument limits of the folded entries
def check_argument_limits():
    """one past each limit of the two entry points of csrc/xconv_bn.hip returns HF_EINVAL before any launch (fake non-null pointers, never
    dereferenced); the limit itself passes the argument check and is stopped by the missing workspace.  Run without a GPU by
    tests/test_xconv_bn_instantiations_cpu.py and on the GPU by tests/test_xconv_bn_abi.py"""
    _lib, L = abi()
    fake = ctypes.c_void_p(256)
    EINVAL, EWS = _lib.HF_EINVAL, _lib.HF_EWORKSPACE

    def fwd(b=2, n=50, p=37, k=8, c0=64, c1=32, m=1, null=None, out=fake):
        ins = [None if i == null else fake for i in range(9)]           # x z1 gamma beta mean invstd fts idx wd
        return L.hf_xconv_depthwise_gather_bn(b, n, p, k, c0, c1, m, *ins, out, None)

    def bwd(b=2, n=50, p=37, k=8, c0=64, c1=32, m=1, null=None, inv=(fake, fake), grads=(fake, fake, fake, fake), sums=(fake, fake), ws=None, nbytes=0):
        ins = [None if i == null else fake for i in range(10)]          # ... and grad_out
        return L.hf_xconv_depthwise_gather_bn_grad(b, n, p, k, c0, c1, m, *ins, *inv, *grads, *sums, ws, nbytes, None)

    bad = {}
    for name, f in (("fwd", fwd), ("bwd", bwd)):
        bad.update({"%s: c0 = 48" % name: f(c0=48), "%s: c0 = 0" % name: f(c0=0), "%s: c1 = 0" % name: f(c1=0), "%s: n_src = 0" % name: f(n=0),
                    "%s: (8, 3)" % name: f(m=3), "%s: (8, 8)" % name: f(m=8), "%s: (4, 1)" % name: f(k=4), "%s: (12, 1)" % name: f(k=12),
                    "%s: b < 0" % name: f(b=-1),
                    "%s: rows k c = 2^32" % name: f(b=1024, p=1024, c0=256, c1=256), "%s: table rows x c = 2^32" % name: f(b=1024, n=8192, p=1, c0=256, c1=256)})
        bad.update({"%s: input %d is NULL" % (name, i): f(null=i) for i in range(9)})
    bad.update({"fwd: no output": fwd(out=None), "bwd: no grad_out": bwd(null=9), "bwd: nothing asked for": bwd(grads=(None,) * 4),
                "bwd: grad_fts without the inverse table": bwd(inv=(None, None)), "bwd: grad_f without dgamma": bwd(sums=(None, fake)),
                "bwd: grad_f without dbeta": bwd(sums=(fake, None))})
    wrong = {name: got for name, got in bad.items() if got != EINVAL}
    assert not wrong, wrong
    # the limits themselves: only the workspace is left to refuse
    limits = dict(plain=bwd(), m2=bwd(m=2), m4=bwd(m=4), c0_128=bwd(c0=128), rows=bwd(b=1024, p=1023, c0=256, c1=256), table=bwd(b=1024, n=8191, p=1, c0=256, c1=256))
    assert set(limits.values()) == {EWS}, limits
    need = L.hf_xconv_depthwise_gather_bn_grad_workspace(2, 37, 8, 64, 32, 1)
    plain = L.hf_xconv_depthwise_gather_grad_workspace(2, 37, 8, 64, 32, 1)
    assert need > plain, (need, plain)
    short = bwd(ws=fake, nbytes=need - 1)
    assert short == EWS, "a workspace one byte short: %d" % short
    no_f = bwd(grads=(fake, None, fake, fake), sums=(None, None))
    assert no_f == EWS, "without grad_f the two sums are not required: %d" % no_f
    empty = L.hf_xconv_depthwise_gather_bn_grad_workspace(0, 37, 8, 64, 32, 1)
    assert empty == 0, "an empty batch needs no workspace: %d" % empty
    status = fwd(b=0)
    assert status == _lib.HF_OK, "an empty batch launches nothing: %d" % status
