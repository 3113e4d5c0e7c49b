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
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xconv_cases as xc  # noqa: E402
from abi_harness import SENTINEL, Arena, In, Out, abi, call, parity_report  # noqa: E402
from xconv_runs import compare, dense_f, is_exact, run_bwd  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
parity_report = parity_report("XCONV_PARITY_OUT", ("hf_xconv", "hf_depthwise"))        # the source of profiles/xconv_parity.md


# ------------------------------------------------------------------------------------------------------- fused forward
def run_fwd(c, t):
    _lib, L = abi()
    sp = _lib.stream_ptr()
    rows, k, m, ch = xc.rows_of(c), c["k"], c["m"], c["c0"] + c["c1"]
    a = Arena(DEV)
    x, wd = In(DEV, t["x"]), In(DEV, t["wd"])
    out = Out(a, rows * ch * m, off="out" in c["off"])
    if c["gather"]:
        fd, fts, idx = In(DEV, t["fd"], "f" in c["off"]), In(DEV, t["fts"], "fts" in c["off"]), In(DEV, t["idx"])
        call(L.hf_xconv_depthwise_gather(c["b"], c["n"], c["p"], k, c["c0"], c["c1"], m, x.p, fd.p, fts.p, idx.p, wd.p, out.p, sp), "hf_xconv_depthwise_gather")
    else:
        f = In(DEV, dense_f(c, t), "f" in c["off"])
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
    _lib, L = abi()
    sp = _lib.stream_ptr()
    rows, k, ch = c["rows"], c["k"], c["c"]
    a = Arena(DEV)
    x, f = In(DEV, t["x"]), In(DEV, t["f"])
    if c["kind"] == "apply":
        out = Out(a, rows * k * ch)
        call(L.hf_xconv_apply(rows, k, ch, x.p, f.p, out.p, sp), "hf_xconv_apply")
        a.check()
        return dict(out=out.view)
    go = In(DEV, t["go"])
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
    _lib, L = abi()
    sp = _lib.stream_ptr()
    rows, k, m, ch = c["rows"], c["k"], c["m"], c["c"]
    a = Arena(DEV)
    x, w = In(DEV, t["x"]), In(DEV, t["w"])
    if c["kind"] == "dw":
        y = Out(a, rows * ch * m)
        call(L.hf_depthwise_k(rows, k, ch, m, x.p, w.p, y.p, sp), "hf_depthwise_k")
        a.check()
        return dict(y=y.view)
    go = In(DEV, t["go"])
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
