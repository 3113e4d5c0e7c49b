"""Kernel-level parity of csrc/xconv.hip through the C ABI against plain fp64 numpy formulas: every kernel, template instantiation and
launch regime (the case table, the restated launch geometry, the references and the bounds are in tests/xconv_cases.py), ctypes on
_lib.lib() with no Python routing in between.

Two input families.  EXACT: small integers, every partial sum an integer below 2^24, so the fp32 result equals fp64 bit for bit whatever
the order of the adds: a dropped row, a row visited twice, a wrong block edge or a misrouted channel shows at any size.  ROUND: seeded
normals, every element within n u M of fp64 (derived in xconv_cases.py; nothing is measured).
Every output is a slice of a sentinel-filled buffer, pre-filled with NaN and checked after the call (a write outside it, or an element
never written, shows); every float input lies between NaN bands (a read outside it that reaches a result shows); the buffers of the
gradients that are not asked for are passed as NULL and must keep their sentinel.  The staging region of the workspace is overwritten
on the staged route of the table gradient and untouched on the direct one, and both routes give the same bits."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xconv_cases as xc  # noqa: E402
import test_bn_abi as bn_abi  # noqa: E402
from test_bn_abi import GUARD, SENTINEL, Arena, within  # noqa: E402
from test_gemm_abi import same  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _abi():
    from heterofusionrcnn_amd import _lib
    return _lib, _lib.lib()


def call(status, name):
    _lib, _ = _abi()
    _lib.check(status, name)


@pytest.fixture(scope="module", autouse=True)
def parity_report():
    """XCONV_PARITY_OUT=<file>: the worst ratios of the session as JSON (the source of profiles/xconv_parity.md)"""
    yield
    path = os.environ.get("XCONV_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"%s|%s" % k: v for k, v in sorted(bn_abi.RATIOS.items()) if k[0].startswith(("hf_xconv", "hf_depthwise"))}, f, indent=1)


class In:
    """an input on the device between two bands of GUARD elements (NaN for floats), 16-byte aligned or (off) one float past that"""

    def __init__(self, a, off=False):
        a = np.ascontiguousarray(a)
        start = GUARD + (1 if off else 0)
        if a.dtype == np.float32:
            self.buf = torch.full((start + a.size + GUARD,), NAN, dtype=torch.float32, device=DEV)
        else:
            assert a.dtype == np.int32
            self.buf = torch.zeros(start + a.size + GUARD, dtype=torch.int32, device=DEV)
        if a.size:
            self.buf[start:start + a.size].copy_(torch.from_numpy(a.reshape(-1)))
        self.p = ctypes.c_void_p(self.buf.data_ptr() + 4 * start)
        assert (self.p.value % 16 == 4) if off else (self.p.value % 16 == 0)


class Out:
    """an output of `n` floats inside a sentinel-filled buffer of the arena, pre-filled with NaN; passed=False: the buffer of a gradient
    that is not asked for (NULL goes to the library) keeps the sentinel everywhere"""

    def __init__(self, arena, n, passed=True, off=False, fill=NAN):
        self.view = arena.out((n,), off=off)
        self.passed = passed
        if passed:
            self.view.fill_(fill)
        self.p = ctypes.c_void_p(self.view.data_ptr()) if passed and n else None
        if passed and n:
            assert (self.p.value % 16 == 4) if off else (self.p.value % 16 == 0)


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def compare(c, got, want, mag, n, name):
    """exact: bit for bit against fp64 rounded once; rounding: within n u M"""
    want = dev64(want).reshape(got.shape)
    if c["family"] == "exact":
        same(got, want, name)
    else:
        b = dev64(xc.bound(n, mag)).reshape(got.shape)
        within(got, want, b, name, c["family"])


def is_exact(c):
    return c["family"] == "exact"


def dense_f(c, t):
    return xc.concat_f(c, t).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- fused forward
def run_fwd(c, t):
    _lib, L = _abi()
    sp = _lib.stream_ptr()
    rows, k, m, ch = xc.rows_of(c), c["k"], c["m"], c["c0"] + c["c1"]
    a = Arena()
    x, wd = In(t["x"]), In(t["wd"])
    out = Out(a, rows * ch * m, off="out" in c["off"])
    if c["gather"]:
        fd, fts, idx = In(t["fd"], "f" in c["off"]), In(t["fts"], "fts" in c["off"]), In(t["idx"])
        call(L.hf_xconv_depthwise_gather(c["b"], c["n"], c["p"], k, c["c0"], c["c1"], m, x.p, fd.p, fts.p, idx.p, wd.p, out.p, sp), "hf_xconv_depthwise_gather")
    else:
        f = In(dense_f(c, t), "f" in c["off"])
        call(L.hf_xconv_depthwise(rows, k, ch, m, x.p, f.p, wd.p, out.p, sp), "hf_xconv_depthwise")
    a.check()
    return out.view


@pytest.mark.parametrize("c", xc.cases_of("fwd"), ids=xc.case_id)
def test_xconv_depthwise_forward(c):
    t = xc.make_inputs(c)
    got = run_fwd(c, t)
    name = "hf_xconv_depthwise%s.out" % ("_gather" if c["gather"] else "")
    mag = None if is_exact(c) else xc.ref_fused_fwd(c, t, mag=True)
    compare(c, got, xc.ref_fused_fwd(c, t), mag, xc.roundings(c)["out"], name)


# ------------------------------------------------------------------------------------------------------- fused backward
BWD_SHAPES = dict(x=lambda c: xc.rows_of(c) * c["k"] * c["k"], f=lambda c: xc.rows_of(c) * c["k"] * (c["c0"] if c["gather"] else c["c0"] + c["c1"]),
                  wd=lambda c: c["k"] * (c["c0"] + c["c1"]) * c["m"], fts=lambda c: c["b"] * c["n"] * c["c1"])


def run_bwd(c, t, ws=None):
    """-> (dict of the gradients, route seen in the workspace: 'staged' / 'direct' / None)"""
    _lib, L = _abi()
    sp = _lib.stream_ptr()
    rows, k, m, c0, c1 = xc.rows_of(c), c["k"], c["m"], c["c0"], c["c1"]
    ws = c["ws"] if ws is None else ws
    a = Arena()
    x, wd, go = In(t["x"]), In(t["wd"]), In(t["go"], "go" in c["off"])
    names = xc.ALL4 if c["gather"] else xc.ALL4[:3]
    g = {n: Out(a, BWD_SHAPES[n](c), passed=n in c["want"], off=(n == "fts" and "gfts" in c["off"])) for n in names}
    seen = None
    if c["gather"]:
        fd, fts, idx, off, ent = In(t["fd"]), In(t["fts"]), In(t["idx"]), In(t["offsets"]), In(t["entries"])
        nbytes = L.hf_xconv_depthwise_gather_grad_workspace(c["b"], c["p"], k, c0, c1, m) if ws else 0
        assert nbytes == (xc.gather_grad_workspace(c["b"], c["p"], k, c0, c1, m) if ws else 0)
        w = Out(a, nbytes // 4, passed=bool(ws and nbytes), fill=SENTINEL)
        call(L.hf_xconv_depthwise_gather_grad(c["b"], c["n"], c["p"], k, c0, c1, m, x.p, fd.p, fts.p, idx.p, wd.p, go.p, off.p, ent.p, g["x"].p, g["f"].p,
                                              g["fts"].p, g["wd"].p, w.p, nbytes, sp), "hf_xconv_depthwise_gather_grad")
        if ws and nbytes and rows:
            block = w.view[:rows * k * c1]
            kept = block == SENTINEL
            seen = "direct" if bool(kept.all()) else "staged"
            assert seen == "direct" or not bool(kept.any()), "the staging region is partly written"
    else:
        f = In(dense_f(c, t))
        call(L.hf_xconv_depthwise_grad(rows, k, c0 + c1, m, x.p, f.p, wd.p, go.p, g["x"].p, g["f"].p, g["wd"].p, sp), "hf_xconv_depthwise_grad")
    a.check()
    for n in names:
        if not g[n].passed:
            assert bool((g[n].view == SENTINEL).all()), "grad_%s was not asked for and was written" % n
    return {n: g[n].view for n in names if g[n].passed}, seen


def check_bwd(c, t, got):
    ref = xc.ref_fused_bwd(c, t, c["want"])
    mag = {} if is_exact(c) else xc.ref_fused_bwd(c, t, c["want"], mag=True)
    n = xc.roundings(c, t)
    entry = "hf_xconv_depthwise%s_grad" % ("_gather" if c["gather"] else "")
    for name in got:
        compare(c, got[name], ref[name], mag.get(name), n[name], "%s.grad_%s" % (entry, name))


@pytest.mark.parametrize("c", xc.cases_of("bwd"), ids=xc.case_id)
def test_xconv_depthwise_backward(c):
    t = xc.make_inputs(c)
    got, seen = run_bwd(c, t)
    assert set(got) == set(c["want"]) & set(xc.ALL4 if c["gather"] else xc.ALL4[:3])
    if xc.rows_of(c) == 0:
        for name in got:
            assert bool((got[name] == 0).all()), "rows == 0: grad_%s comes back as zeros" % name
        return
    if c["gather"] and c["ws"]:
        assert seen == (xc.route(c) or "direct"), "the route xdw_fts_direct documents for the shape"
    check_bwd(c, t, got)
    if xc.route(c) == "staged":                 # the other route: same bits
        other, _ = run_bwd(dict(c, want=("fts",)), t, ws=False)
        assert torch.equal(other["fts"], got["fts"]), "staged and direct table gradients differ"


# ------------------------------------------------------------------------------------------------------- two-kernel entry points
def run_apply(c, t):
    _lib, L = _abi()
    sp = _lib.stream_ptr()
    rows, k, ch = c["rows"], c["k"], c["c"]
    a = Arena()
    x, f = In(t["x"]), In(t["f"])
    if c["kind"] == "apply":
        out = Out(a, rows * k * ch)
        call(L.hf_xconv_apply(rows, k, ch, x.p, f.p, out.p, sp), "hf_xconv_apply")
        a.check()
        return dict(out=out.view)
    go = In(t["go"])
    g = dict(x=Out(a, rows * k * k, passed="x" in c["want"]), f=Out(a, rows * k * ch, passed="f" in c["want"]))
    call(L.hf_xconv_apply_grad(rows, k, ch, x.p, f.p, go.p, g["x"].p, g["f"].p, sp), "hf_xconv_apply_grad")
    a.check()
    for n in g:
        if not g[n].passed:
            assert bool((g[n].view == SENTINEL).all())
    return {n: g[n].view for n in g if g[n].passed}


@pytest.mark.parametrize("c", xc.cases_of("apply", "apply_grad"), ids=xc.case_id)
def test_xconv_apply(c):
    t = xc.make_inputs(c)
    got = run_apply(c, t)
    n = xc.roundings(c)
    if c["kind"] == "apply":
        compare(c, got["out"], xc.ref_apply(t), None if is_exact(c) else xc.ref_apply(t, mag=True), n["out"], "hf_xconv_apply.out")
        return
    ref, mag = xc.ref_apply_grad(t), ({} if is_exact(c) else xc.ref_apply_grad(t, mag=True))
    assert set(got) == set(c["want"])
    for name in got:
        compare(c, got[name], ref[name], mag.get(name), n[name], "hf_xconv_apply_grad.grad_%s" % name)


def run_dw(c, t):
    _lib, L = _abi()
    sp = _lib.stream_ptr()
    rows, k, m, ch = c["rows"], c["k"], c["m"], c["c"]
    a = Arena()
    x, w = In(t["x"]), In(t["w"])
    if c["kind"] == "dw":
        y = Out(a, rows * ch * m)
        call(L.hf_depthwise_k(rows, k, ch, m, x.p, w.p, y.p, sp), "hf_depthwise_k")
        a.check()
        return dict(y=y.view)
    go = In(t["go"])
    g = dict(x=Out(a, rows * k * ch, passed="x" in c["want"]), w=Out(a, k * ch * m, passed="w" in c["want"]))
    if c["ws"]:
        nbytes = L.hf_depthwise_k_grad_workspace(rows, k, ch, m)
        assert nbytes == xc.dw_grad_workspace(rows, k, ch, m)
        ws = Out(a, nbytes // 4, fill=SENTINEL)
        call(L.hf_depthwise_k_grad_ws(rows, k, ch, m, x.p, w.p, go.p, g["x"].p, g["w"].p, ws.p, nbytes, sp), "hf_depthwise_k_grad_ws")
    else:
        call(L.hf_depthwise_k_grad(rows, k, ch, m, x.p, w.p, go.p, g["x"].p, g["w"].p, sp), "hf_depthwise_k_grad")
    a.check()
    for n in g:
        if not g[n].passed:
            assert bool((g[n].view == SENTINEL).all())
    return {n: g[n].view for n in g if g[n].passed}


@pytest.mark.parametrize("c", xc.cases_of("dw", "dw_grad"), ids=xc.case_id)
def test_depthwise_k(c):
    t = xc.make_inputs(c)
    got = run_dw(c, t)
    n = xc.roundings(c)
    if c["kind"] == "dw":
        compare(c, got["y"], xc.ref_dw(t), None if is_exact(c) else xc.ref_dw(t, mag=True), n["y"], "hf_depthwise_k.y")
        return
    ref, mag = xc.ref_dw_grad(t), ({} if is_exact(c) else xc.ref_dw_grad(t, mag=True))
    assert set(got) == set(c["want"])
    entry = "hf_depthwise_k_grad" + ("_ws" if c["ws"] else "")
    for name in got:
        compare(c, got[name], ref[name], mag.get(name), n[name], "%s.grad_%s" % (entry, name))


# ------------------------------------------------------------------------------------------------------- determinism with a workspace
def _deterministic_cases():
    """seeded normals (with integers any order gives the same bits) at shapes on every reduction path that ends in a workspace: the fused
    weight gradient in blocks of 4, of 32 and of 33 rows; depthwise_dw_kernel by shuffles, by LDS turns and with one slot"""
    out = []
    for c in xc.all_cases():
        if c["family"] != "exact" or not c.get("ws"):
            continue
        if c["kind"] == "bwd" and c["gather"] and "wd" in c["want"] and c["regime"] in ("rows_le_32", "floor32", "ragged_blocks", "staged") and c["k"] != 4:
            out.append(dict(c, family="round", want=("wd",)))
        if c["kind"] == "dw_grad" and c["regime"].startswith("dw_") and c["rows"] in (65, 203):
            out.append(dict(c, family="round"))
    return out


@pytest.mark.parametrize("c", _deterministic_cases(), ids=xc.case_id)
def test_weight_gradient_with_a_workspace_is_deterministic(c):
    """include/hfops.h: with a workspace the weight gradient is added in a fixed order.  Three calls, the same bits"""
    t = xc.make_inputs(c)
    run = (lambda: run_bwd(c, t)[0]["wd"]) if c["kind"] == "bwd" else (lambda: run_dw(c, t)["w"])
    first = run().clone()
    for _ in range(2):
        again = run()
        assert torch.equal(first, again), "%d of %d elements differ between two calls" % (int((first != again).sum()), first.numel())


def test_deterministic_cases_cover_every_reduction_path():
    cs = _deterministic_cases()
    assert {xc.dw_reduction(c["c"]) for c in cs if c["kind"] == "dw_grad"} == {"shuffle", "lds", "one_slot"}
    assert {c["regime"] for c in cs if c["kind"] == "bwd"} == {"rows_le_32", "floor32", "ragged_blocks", "staged"}


def render_parity(report):
    """profiles/xconv_parity.md's table from the JSON that a session with XCONV_PARITY_OUT wrote"""
    lines = ["| output | family | worst ratio | |", "|---|---|---:|---|"]
    for key, v in sorted(report.items()):
        name, fam = key.split("|")
        lines.append("| `%s` | %s | %.3g | %s |" % (name, fam, v, "**>= 0.5**" if v >= 0.5 else ""))
    return "\n".join(lines)


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        print(render_parity(json.load(f)))
