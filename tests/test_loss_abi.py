"""Kernel-level parity of the fused loss entry points of csrc/glue.hip through the C ABI against plain fp64 numpy formulas:
hf_rpn_loss_fwd / _bwd and hf_rcnn_loss_fwd / _bwd at every launch regime, limit and mask branch (the case table, the restated launch
rule, the references and the bounds are in tests/loss_cases.py), ctypes on _lib.lib() with no Python routing in between.

Every float input lies between NaN bands (a read outside it that reaches a result shows).  out5 / out6, the logit gradient and grad_head
are slices of sentinel-filled buffers, pre-filled with NaN and checked after the call: a write outside them or an element never written
shows, and so does a missing zero-fill (every grad_head element that no formula reaches, every logit-gradient row that is ignored or
unmasked, must be exactly 0.0).  The forward workspace is exactly hf_*_loss_workspace() bytes of NaN inside guards.  The backward reads
the out5 / out6 that the forward call wrote on the device.  Every case is called twice and must give the same bits (no atomics)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as lc  # noqa: E402
from abi_harness import SENTINEL, Arena, In, Out, abi, call, parity_report, same_bits, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
parity_report = parity_report("LOSS_PARITY_OUT", ("hf_rpn_loss", "hf_rcnn_loss"))       # the source of profiles/loss_parity.md
ENTRY = {"rpn": ("hf_rpn_loss_fwd", "hf_rpn_loss_bwd"), "rcnn": ("hf_rcnn_loss_fwd", "hf_rcnn_loss_bwd")}


def scalars(c):
    """the float arguments between the targets and the outputs"""
    return tuple(c["weights"]) if c["kind"] == "rpn" else tuple(c["thresholds"]) + tuple(c["weights"])


def run_case(c, t):
    """forward, then backward on the out5 / out6 that the forward left on the device -> host copies of out, the logit gradient and
    grad_head (rows == 0: the two gradient buffers, eight sentinels each, as the backward left them)"""
    _lib, L = abi()
    sp = _lib.stream_ptr()
    kind, rows, k, nbx, nbt, off = c["kind"], c["rows"], c["k"], c["nbx"], c["nbt"], c["off"]
    k1, d = k + 1, lc.head_width(nbx, nbt)
    fwd, bwd = ENTRY[kind]
    names = lc.RPN_ARGS if kind == "rpn" else lc.RCNN_ARGS
    a = Arena(DEV)
    args = [In(DEV, t[n], off and t[n].dtype == np.float32) for n in names]
    ptrs = [x.p for x in args]
    out = Out(a, len(lc.OUT_NAMES[kind]), off=off)
    nbytes = getattr(L, "hf_%s_loss_workspace" % kind)()
    assert nbytes == (lc.rpn_workspace() if kind == "rpn" else lc.rcnn_workspace())
    ws = Out(a, nbytes // 4)
    call(getattr(L, fwd)(rows, k, nbx, nbt, *ptrs, *scalars(c), out.p, ws.p, nbytes, sp), fwd)
    up = In(DEV, np.array([c["upstream"]], np.float32), off)
    if rows:
        g_logits, g_head = Out(a, rows * k1, off=off), Out(a, rows * k * d, off=off)
    else:
        g_logits, g_head = Out(a, 8, fill=SENTINEL), Out(a, 8, fill=SENTINEL)
    call(getattr(L, bwd)(rows, k, nbx, nbt, *ptrs, *scalars(c), out.p, up.p, g_logits.p, g_head.p, sp), bwd)
    a.check()
    host = lambda v, shape: v.view.cpu().numpy().reshape(shape)
    if rows == 0:
        return dict(out=host(out, -1), grad_logits=host(g_logits, -1), grad_head=host(g_head, -1))
    return dict(out=host(out, -1), grad_logits=host(g_logits, (rows, k1)), grad_head=host(g_head, (rows, k, d)))


def close(got, want, bound, name):
    b = np.asarray(bound, np.float64)
    within(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want)), torch.from_numpy(b.reshape((1,) * got.ndim) if b.ndim == 0 else b),
           name, "round")


def check_case(c):
    kind = c["kind"]
    fwd, bwd = ENTRY[kind]
    t = lc.make_inputs(c)
    got, again = run_case(c, t), run_case(c, t)
    for key in got:
        assert same_bits(got[key], again[key]), "%s differs between two calls" % key
    if c["rows"] == 0:
        assert (got["out"] == 0).all(), "rows == 0: the forward writes zeros"
        assert (got["grad_logits"] == SENTINEL).all() and (got["grad_head"] == SENTINEL).all(), "rows == 0: the backward writes nothing"
        return
    r64, r32 = lc.REF[kind](c, t), lc.REF[kind](c, t, np.float32)
    names = lc.OUT_NAMES[kind]
    ncount = len(r64["counts"])
    print("%s: out = %s, reference %s" % (fwd, got["out"].tolist(), r64["out"].tolist()))
    assert got["out"][3:3 + ncount].tolist() == [float(n) for n in r64["counts"]], "the counts are exact"
    bound = lc.forward_bounds(c, r64, r32)
    for i, name in enumerate(names):
        if not 3 <= i < 3 + ncount:
            close(got["out"][i:i + 1], r64["out"][i:i + 1], bound[i:i + 1], "%s.%s" % (fwd, name))
    for key, ref, live in (("grad_logits", lc.LOGIT_GRAD[kind], lc.LOGIT_LIVE[kind]), ("grad_head", "grad_head", "live_head")):
        g = got[key]
        name = "%s.%s" % (bwd, ref)
        assert not np.isnan(g).any(), "%s: %d elements never written" % (name, int(np.isnan(g).sum()))
        mask = r64[live] if r64[live].ndim == g.ndim else np.broadcast_to(r64[live][:, None], g.shape)
        assert (g[~mask] == 0).all(), "%s: %d elements that no formula reaches are not exactly 0.0" % (name, int((g[~mask] != 0).sum()))
        close(g, r64[ref], lc.grad_bound(r32[ref], r64[ref]), name)


@pytest.mark.parametrize("c", lc.cases_of("rpn"), ids=lc.case_id)
def test_rpn_loss(c):
    check_case(c)


@pytest.mark.parametrize("c", lc.cases_of("rcnn"), ids=lc.case_id)
def test_rcnn_loss(c):
    check_case(c)


def test_rejected_calls_write_nothing():
    """the argument checks of tests/test_abi.py (which need no GPU) with real buffers: a short workspace and a count past the register
    arrays return before anything is launched, out5 / out6 and both gradients keep their sentinels"""
    _lib, L = abi()
    sp = _lib.stream_ptr()
    for kind in ("rpn", "rcnn"):
        c = next(c for c in lc.cases_of(kind) if c["rows"] == 257 and not c["off"])
        t = lc.make_inputs(c)
        rows, k, nbx, nbt = c["rows"], c["k"], c["nbx"], c["nbt"]
        fwd, bwd = (getattr(L, n) for n in ENTRY[kind])
        a = Arena(DEV)
        ptrs = [In(DEV, t[n]).p for n in (lc.RPN_ARGS if kind == "rpn" else lc.RCNN_ARGS)]
        nbytes = getattr(L, "hf_%s_loss_workspace" % kind)()
        out, ws, up = Out(a, 6, fill=SENTINEL), Out(a, nbytes // 4, fill=SENTINEL), In(DEV, np.ones(1, np.float32))
        gl, gh = Out(a, rows * (k + 1), fill=SENTINEL), Out(a, rows * k * lc.head_width(nbx, nbt), fill=SENTINEL)
        s = scalars(c)
        assert fwd(rows, k, nbx, nbt, *ptrs, *s, out.p, ws.p, nbytes - 1, sp) == _lib.HF_EWORKSPACE
        assert fwd(rows, k, nbx, nbt, *ptrs, *s, out.p, None, nbytes, sp) == _lib.HF_EWORKSPACE
        assert fwd(rows, 8, nbx, nbt, *ptrs, *s, out.p, ws.p, nbytes, sp) == _lib.HF_EINVAL
        assert fwd(rows, k, 33, nbt, *ptrs, *s, out.p, ws.p, nbytes, sp) == _lib.HF_EINVAL
        assert bwd(rows, k, nbx, 33, *ptrs, *s, out.p, up.p, gl.p, gh.p, sp) == _lib.HF_EINVAL
        assert bwd(rows, k, nbx, nbt, *ptrs, *s, out.p, None, gl.p, gh.p, sp) == _lib.HF_EINVAL
        assert bwd(-1, k, nbx, nbt, *ptrs, *s, out.p, up.p, gl.p, gh.p, sp) == _lib.HF_EINVAL
        a.untouched()


def render_parity(report):
    """profiles/loss_parity.md from the JSON that a session with LOSS_PARITY_OUT wrote"""
    lines = ["# Parity of the fused loss kernels of csrc/glue.hip with fp64 through the C ABI", "",
             "Worst `|got - ref64| / bound` of every output over the cases of `tests/loss_cases.py`, one MI355X session of",
             "`LOSS_PARITY_OUT=report.json pytest -m gpu tests/test_loss_abi.py`; rendered by `python tests/test_loss_abi.py report.json`.",
             "The bounds are those derived in `tests/loss_cases.py`; the counts (`#fg`, `#cls`, `#reg`) and the structural zeros are compared",
             "exactly and do not appear.  Every ratio must be <= 1; those >= 0.5 are marked.  No tolerance is tuned from this file.", "",
             "| output | worst ratio | |", "|---|---:|---|"]
    for key, v in sorted(report.items()):
        lines.append("| `%s` | %.3g | %s |" % (key.split("|")[0], v, "**>= 0.5**" if v >= 0.5 else ""))
    return "\n".join(lines)


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        print(render_parity(json.load(f)))
