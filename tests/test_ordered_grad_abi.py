"""The ordered image-feature gradients through the C ABI (ctypes on _lib.lib(), no Python routing in between) against the sequential
fp32 references of tests/ordered_grad_cases.py: hf_project_gather_grad_ordered on every project case, hf_crop_and_resize_grad_ordered on
every entry of roi_image_cases.CROP_CASES with the two bad box_ind rows appended.  Inputs sit between NaN bands, the map is a slice of a
sentinel-filled buffer pre-filled with NaN (an element never written shows).  EQUAL BITS with the reference, the sign of zero
included; three calls repeat them; against the atomic entry on the same inputs: equal bits at every pixel with at most two entries, within
(k + 4) 2^-24 sum|g| elsewhere; a workspace one byte short is HF_EINVAL and writes nothing; where c % 4 == 0 also with grad_out and the
map one float past a 16-byte boundary (the one-float-per-lane reduce instead of the 16-byte one); one case of each op is captured as a single
chain and replayed three times with grad_out rewritten in place (counters left over from a replay would show)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ordered_grad_cases as oc  # noqa: E402
import roi_image_cases as rc  # noqa: E402
from abi_harness import Arena, In, Out, abi, call, dev64  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def inp(a, off=False):
    return In(DEV, a.copy(), off)


def same_bits(got, want, name):
    want = torch.from_numpy(np.array(want)).cuda().reshape(got.shape)
    differ = got.contiguous().view(torch.int32) != want.view(torch.int32)          # a NaN left from the prefill differs too
    assert not bool(differ.any()), "%s: %d of %d elements differ in their bits from the sequential fp32 sum" % (name, int(differ.sum()), got.numel())


def workspace(nbytes):
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    return ws


def run_project(name, ordered=True, short=0, off=False):
    _lib, L = abi()
    b, p, h, w, c = oc.PROJECT_CASES[name]
    t = oc.make_project(name)
    a = Arena(DEV)
    go, pix = inp(t["go"], off), inp(t["pix"])
    grad = Out(a, b * h * w * c, off=off)
    if ordered:
        need = L.hf_project_gather_grad_ordered_workspace(b, p, h, w, c)
        ws = workspace(need)
        status = L.hf_project_gather_grad_ordered(b, p, h, w, c, go.p, pix.p, grad.p, ctypes.c_void_p(ws.data_ptr()), need - short,
                                                  _lib.stream_ptr())
        if short:
            torch.cuda.synchronize()
            assert status == _lib.HF_EINVAL and bool(torch.isnan(grad.view).all())
            return None
        call(status, "hf_project_gather_grad_ordered")
    else:
        call(L.hf_project_gather_grad(b, p, h, w, c, go.p, pix.p, grad.p, _lib.stream_ptr()), "hf_project_gather_grad")
    a.check()
    return grad.view.reshape(b, h, w, c)


def run_crop(name, ordered=True, short=0, off=False):
    _lib, L = abi()
    d, t = rc.dims(name), rc.make_inputs(name, True)
    n = t["boxes"].shape[0]
    a = Arena(DEV)
    go, boxes, ind = inp(t["go"], off), inp(t["boxes"]), inp(t["ind"])
    grad = Out(a, t["img"].size, off=off)
    dims = (d["b"], d["h"], d["w"], d["c"], n, d["ch"], d["cw"])
    if ordered:
        need = L.hf_crop_and_resize_grad_ordered_workspace(*dims)
        ws = workspace(need)
        status = L.hf_crop_and_resize_grad_ordered(*dims, go.p, boxes.p, ind.p, grad.p, ctypes.c_void_p(ws.data_ptr()), need - short,
                                                   _lib.stream_ptr())
        if short:
            torch.cuda.synchronize()
            assert status == _lib.HF_EINVAL and bool(torch.isnan(grad.view).all())
            return None
        call(status, "hf_crop_and_resize_grad_ordered")
    else:
        call(L.hf_crop_and_resize_grad(*dims, go.p, boxes.p, ind.p, grad.p, _lib.stream_ptr()), "hf_crop_and_resize_grad")
    a.check()
    return grad.view.reshape(t["img"].shape)


def against_the_atomic_entry(got, atomic, k, want64, bound, name):
    few = torch.from_numpy(np.broadcast_to((k <= 2)[..., None], tuple(got.shape)).copy()).cuda()
    differ = (got.contiguous().view(torch.int32) != atomic.contiguous().view(torch.int32)) & few
    assert not bool(differ.any()), "%s: %d elements of pixels with at most two entries differ from the atomic entry" % (name, int(differ.sum()))
    want64, bound = dev64(DEV, want64.copy()), dev64(DEV, bound.copy())
    for what, x in (("ordered", got), ("atomic", atomic)):
        worst = float(((x.double() - want64).abs() / bound.clamp(min=1e-300)).max()) if x.numel() else 0.0
        print("%s %s: max |got - ref64| / bound = %.3g" % (name, what, worst))
        assert bool(((x.double() - want64).abs() <= bound).all()), "%s: the %s entry leaves the bound" % (name, what)
    assert bool(((got.double() - atomic.double()).abs() <= bound).all()), "%s: the two entries are further apart than the bound" % name


@pytest.mark.parametrize("name", list(oc.PROJECT_CASES))
def test_project_gather_grad_ordered(name):
    b, p, h, w, c = oc.PROJECT_CASES[name]
    r = oc.project_reference(name)
    got = run_project(name)
    same_bits(got, r["grad"], "hf_project_gather_grad_ordered." + name)
    for _ in range(2):
        assert torch.equal(got.contiguous().view(torch.int32), run_project(name).contiguous().view(torch.int32)), "two calls differ"
    if b:
        against_the_atomic_entry(got, run_project(name, ordered=False), r["k"], r["want64"], r["bound"], "project." + name)
        run_project(name, short=1)
    if b and c % 4 == 0:
        # grad_out and the map one float past a 16-byte boundary take the one-float-per-lane reduce: the same sums, the same bits
        same_bits(run_project(name, off=True), r["grad"], "hf_project_gather_grad_ordered.%s, off the 16-byte boundary" % name)


@pytest.mark.parametrize("name", list(rc.CROP_CASES))
def test_crop_and_resize_grad_ordered(name):
    r, r64 = oc.crop_reference(name, True), rc.reference(name, True)
    got = run_crop(name)
    same_bits(got, r["grad"], "hf_crop_and_resize_grad_ordered." + name)
    for _ in range(2):
        assert torch.equal(got.contiguous().view(torch.int32), run_crop(name).contiguous().view(torch.int32)), "two calls differ"
    against_the_atomic_entry(got, run_crop(name, ordered=False), r["k"], r64["grad"], r64["grad_bound"], "crop." + name)
    run_crop(name, short=1)
    if rc.dims(name)["c"] % 4 == 0:
        same_bits(run_crop(name, off=True), r["grad"], "hf_crop_and_resize_grad_ordered.%s, off the 16-byte boundary" % name)


def _replays(launch, go, rewrite, expect, name):
    """warm up on a side stream, capture `launch` as one chain, replay three times with `go` rewritten in place before each"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = launch()
    for seed in range(3):
        new = rewrite(seed)
        go.copy_(torch.from_numpy(new).cuda().reshape(go.shape))
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        same_bits(out, expect(new), "%s, replay %d" % (name, seed))


def test_project_gather_grad_ordered_replays_in_a_captured_graph():
    _lib, L = abi()
    name = "straddle_c5"
    b, p, h, w, c = oc.PROJECT_CASES[name]
    t = oc.make_project(name)
    go, pix = torch.from_numpy(t["go"].copy()).cuda(), torch.from_numpy(t["pix"].copy()).cuda()
    out = torch.empty(b, h, w, c, device="cuda")
    need = L.hf_project_gather_grad_ordered_workspace(b, p, h, w, c)
    ws = workspace(need)

    def launch():
        call(L.hf_project_gather_grad_ordered(b, p, h, w, c, ctypes.c_void_p(go.data_ptr()), ctypes.c_void_p(pix.data_ptr()),
                                              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), need, _lib.stream_ptr()),
             "hf_project_gather_grad_ordered")
        return out

    def expect(new):
        targets, valid, key, term = oc.entries_project(name, go=new)
        return oc.sequential(targets, valid, key, term)

    _replays(launch, go, lambda seed: oc.order_sensitive_values(np.random.default_rng(100 + seed), (b, p, c)), expect, "project." + name)


def test_crop_and_resize_grad_ordered_replays_in_a_captured_graph():
    _lib, L = abi()
    name = "vec_c32"
    d, t = rc.dims(name), rc.make_inputs(name, True)
    n = t["boxes"].shape[0]
    go, boxes, ind = (torch.from_numpy(t[k].copy()).cuda() for k in ("go", "boxes", "ind"))
    out = torch.empty(t["img"].shape, device="cuda")
    dims = (d["b"], d["h"], d["w"], d["c"], n, d["ch"], d["cw"])
    need = L.hf_crop_and_resize_grad_ordered_workspace(*dims)
    ws = workspace(need)

    def launch():
        call(L.hf_crop_and_resize_grad_ordered(*dims, ctypes.c_void_p(go.data_ptr()), ctypes.c_void_p(boxes.data_ptr()),
                                               ctypes.c_void_p(ind.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                                               ctypes.c_void_p(ws.data_ptr()), need, _lib.stream_ptr()), "hf_crop_and_resize_grad_ordered")
        return out

    def expect(new):
        targets, valid, key, term = oc.entries_crop(t["img"].shape, t["boxes"], t["ind"], new)
        return oc.sequential(targets, valid, key, term)

    _replays(launch, go, lambda seed: oc.order_sensitive_values(np.random.default_rng(200 + seed), t["go"].shape), expect, "crop." + name)
