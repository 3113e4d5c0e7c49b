"""hf_xconv_depthwise_grad_ws (csrc/xconv.hip) through the C ABI: the dense fused X-Conv gradient whose row chunks' partial weight
gradients meet in a workspace and are added in a fixed order.

Reference (fp64, from the contract of include/hfops.h, never from the kernels): P[r] = x[r] f[r] (k x c), out[r][ch m + mm] =
sum_w P[r][w][ch] wd[w][ch][mm], so grad_wd[w][ch][mm] = sum_r P[r][w][ch] go[r][ch m + mm].
Bound per element of grad_wd: a term is P go with P a k-term fp32 dot product (at most k roundings of magnitude
A[r][w][ch] = sum_j |x[r][w][j]| |f[r][j][ch]|) and one product rounding; summing the terms adds, per term, at most as many roundings
as there are additions between it and the result (the depth of the sum).  With u = 2^-24 and M = sum_r A[r][w][ch] |go[r][ch m + mm]|:
  workspace form   |got - ref| <= (rows per chunk + chunks + k + 2) u M: a chunk's rows meet in any order inside their block (depth at
                   most the rows of the chunk), the chunk sums are then added one after the other
  atomic form      |got - ref| <= (n + k + 2) u M: any order over all n rows
For the 1400-row case (elements of size ~100, M ~ 6000) that is 0.03 and 0.5; a dropped row chunk (44 of them, each worth ~16), a
short workspace or a wrong chunk count in the reduction is 500 times outside the first.
grad_x and grad_f take no part in the change: they must be the BITS of hf_xconv_depthwise_grad, and grad_wd of the two entry points
must agree within the sum of the two bounds.  Rows: one chunk (3), several chunks below the 32-row rule (20 = 5 chunks of 4), a ragged last
chunk (77 = 32 + 32 + 13; 1400 = 43 x 32 + 24), one and two channel columns of the grid (c = 40, 72), (k, m) = (8, 2), (8, 1), (4, 4).
Inputs sit between NaN bands, outputs and the workspace are slices of sentinel-filled buffers."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from abi_harness import SENTINEL, Arena, In, Out, abi, call, dev64, within  # noqa: E402

DEV = "cuda"
U = 2.0 ** -24
# name: (rows, k, c, m, expected row chunks)
CASES = {"one_chunk": (3, 8, 40, 2, 1), "five_chunks": (20, 8, 40, 2, 5), "ragged_3": (77, 8, 40, 1, 3), "ragged_44": (1400, 8, 40, 2, 44),
         "two_columns": (77, 8, 72, 2, 3), "k4_m4": (50, 4, 16, 4, 2)}


def make(name):
    rows, k, c, m, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    t = dict(x=rng.standard_normal((rows, k, k)), f=rng.standard_normal((rows, k, c)), wd=rng.standard_normal((k, c, m)),
             go=rng.standard_normal((rows, c * m)))
    return {n: a.astype(np.float32) for n, a in t.items()}


def reference(t, k, c, m):
    """-> (grad_wd fp64 (k,c,m), u M (k,c,m))"""
    x, f, go = (t[n].astype(np.float64) for n in ("x", "f", "go"))
    rows = x.shape[0]
    g = go.reshape(rows, c, m)
    want = np.einsum("rwc,rcm->wcm", np.einsum("rwj,rjc->rwc", x, f), g)
    mag = np.einsum("rwc,rcm->wcm", np.einsum("rwj,rjc->rwc", np.abs(x), np.abs(f)), np.abs(g))
    return want, U * mag


def test_workspace_size_and_argument_checks_without_a_gpu():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(256)
    for rows, k, c, m, chunks in CASES.values():
        assert L.hf_xconv_depthwise_grad_workspace(rows, k, c, m) == 4 * chunks * k * c * m
    assert L.hf_xconv_depthwise_grad_workspace(0, 8, 40, 2) == 0 and L.hf_xconv_depthwise_grad_workspace(-1, 8, 40, 2) == 0
    need = L.hf_xconv_depthwise_grad_workspace(77, 8, 40, 2)
    ws = lambda rows=77, x=one, gx=one, gf=one, gw=one, w=one, nbytes=need: L.hf_xconv_depthwise_grad_ws(
        rows, 8, 40, 2, x, one, one, one, gx, gf, gw, w, nbytes, None)
    assert ws(w=None) == _lib.HF_EWORKSPACE and ws(nbytes=need - 1) == _lib.HF_EWORKSPACE and ws(nbytes=0) == _lib.HF_EWORKSPACE
    assert ws(x=None) == _lib.HF_EINVAL and ws(rows=-1) == _lib.HF_EINVAL and ws(gx=None, gf=None, gw=None) == _lib.HF_EINVAL


def _run(name, with_ws, off=False):
    _lib, L = abi()
    rows, k, c, m, _ = CASES[name]
    t = make(name)
    a = Arena(DEV)
    x, f, wd, go = (In(DEV, t[n]) for n in ("x", "f", "wd", "go"))
    gx, gf, gw = Out(a, rows * k * k), Out(a, rows * k * c, off=off), Out(a, k * c * m)
    if with_ws:
        nbytes = L.hf_xconv_depthwise_grad_workspace(rows, k, c, m)
        ws = Out(a, nbytes // 4)
        call(L.hf_xconv_depthwise_grad_ws(rows, k, c, m, x.p, f.p, wd.p, go.p, gx.p, gf.p, gw.p, ws.p, nbytes, _lib.stream_ptr()),
             "hf_xconv_depthwise_grad_ws")
    else:
        call(L.hf_xconv_depthwise_grad(rows, k, c, m, x.p, f.p, wd.p, go.p, gx.p, gf.p, gw.p, _lib.stream_ptr()), "hf_xconv_depthwise_grad")
    a.check()
    return gx.view.clone(), gf.view.clone(), gw.view.reshape(k, c, m).clone()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_weight_gradient_against_fp64_and_the_atomic_entry_point(name):
    rows, k, c, m, chunks = CASES[name]
    want, um = reference(make(name), k, c, m)
    want, um = dev64(DEV, want), dev64(DEV, um)
    bound_ws, bound = (-(-rows // chunks) + chunks + k + 2) * um, (rows + k + 2) * um
    gx, gf, gw = _run(name, True)
    within(gw, want, bound_ws, "hf_xconv_depthwise_grad_ws." + name, "round")
    for _ in range(2):
        again = _run(name, True)
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip((gx, gf, gw), again)), "two calls differ"
    ax, af, aw = _run(name, False)
    within(aw, want, bound, "hf_xconv_depthwise_grad." + name, "round")
    assert bool(((gw - aw).abs().double() <= bound_ws + bound).all())
    assert torch.equal(gx.view(torch.int32), ax.view(torch.int32)) and torch.equal(gf.view(torch.int32), af.view(torch.int32))
    # grad_f one float past a 16-byte boundary: the same bits everywhere
    assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip((gx, gf, gw), _run(name, True, off=True)))


@pytest.mark.gpu
def test_empty_batch_zero_fills_the_weight_gradient_and_needs_no_workspace():
    _lib, L = abi()
    a = Arena(DEV)
    wd = In(DEV, np.ones((8, 40, 2), np.float32))
    gw = Out(a, 8 * 40 * 2)
    one = ctypes.c_void_p(wd.p.value)           # never read: there are no rows
    call(L.hf_xconv_depthwise_grad_ws(0, 8, 40, 2, one, one, wd.p, one, None, None, gw.p, None, 0, _lib.stream_ptr()), "hf_xconv_depthwise_grad_ws")
    a.check()
    assert bool((gw.view.view(torch.int32) == 0).all())


@pytest.mark.gpu
def test_only_the_weight_gradient_and_only_the_others():
    """grad_wd alone and grad_x / grad_f alone: the same bits as all three together; what is not asked for is not written"""
    _lib, L = abi()
    name = "ragged_3"
    rows, k, c, m, _ = CASES[name]
    t = make(name)
    gx0, gf0, gw0 = _run(name, True)
    nbytes = L.hf_xconv_depthwise_grad_workspace(rows, k, c, m)
    for want_w in (True, False):
        a = Arena(DEV)
        x, f, wd, go = (In(DEV, t[n]) for n in ("x", "f", "wd", "go"))
        gx, gf, gw = Out(a, rows * k * k, passed=not want_w), Out(a, rows * k * c, passed=not want_w), Out(a, k * c * m, passed=want_w)
        ws = Out(a, nbytes // 4, passed=want_w)
        call(L.hf_xconv_depthwise_grad_ws(rows, k, c, m, x.p, f.p, wd.p, go.p, gx.p, gf.p, gw.p, ws.p, nbytes if want_w else 0,
                                          _lib.stream_ptr()), "hf_xconv_depthwise_grad_ws")
        a.check()
        if want_w:
            assert torch.equal(gw.view.view(torch.int32), gw0.reshape(-1).view(torch.int32))
            assert bool((gx.view == SENTINEL).all()) and bool((gf.view == SENTINEL).all())
        else:
            assert torch.equal(gx.view.view(torch.int32), gx0.view(torch.int32)) and torch.equal(gf.view.view(torch.int32), gf0.view(torch.int32))
            assert bool((gw.view == SENTINEL).all()) and bool((ws.view == SENTINEL).all())
