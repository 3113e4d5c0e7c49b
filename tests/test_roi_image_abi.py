"""Kernel-level parity of csrc/roi_image.hip through the C ABI (ctypes on _lib.lib(), no Python routing in between) against the
references and bounds of tests/roi_image_cases.py.  Inputs sit between NaN bands, outputs are slices of sentinel-filled buffers and
are pre-filled with NaN: a read or a write outside a tensor, or an element never written, shows.  The forward and the box projection
are called twice and repeat their bits; the gradient is called twice and each result is within the bound (atomics may reorder the
sums).  Every case carries a row that is not finite, and here also one row with box_ind -1 and one with box_ind b."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roi_image_cases as rc  # noqa: E402
from abi_harness import Arena, In, Out, abi, call, dev64, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def inp(a, off=False):
    """the tables are read-only arrays: torch wants a writable one"""
    return In(DEV, a.copy(), off)


def run_forward(name, t, off=False):
    _lib, L = abi()
    d = rc.dims(name)
    n = t["boxes"].shape[0]
    a = Arena(DEV)
    img, boxes, ind = inp(t["img"], off), inp(t["boxes"]), inp(t["ind"])
    out = Out(a, n * d["ch"] * d["cw"] * d["c"], off=off)
    call(L.hf_crop_and_resize(d["b"], d["h"], d["w"], d["c"], n, d["ch"], d["cw"], img.p, boxes.p, ind.p, d["extrap"], out.p,
                              _lib.stream_ptr()), "hf_crop_and_resize")
    a.check()
    return out.view.reshape(n, d["ch"], d["cw"], d["c"])


def run_backward(name, t, off=False):
    _lib, L = abi()
    d = rc.dims(name)
    n = t["boxes"].shape[0]
    a = Arena(DEV)
    go, boxes, ind = inp(t["go"]), inp(t["boxes"]), inp(t["ind"])
    grad = Out(a, t["img"].size, off=off)                         # pre-filled with NaN: a missing zero fill shows
    call(L.hf_crop_and_resize_grad(d["b"], d["h"], d["w"], d["c"], n, d["ch"], d["cw"], go.p, boxes.p, ind.p, grad.p,
                                   _lib.stream_ptr()), "hf_crop_and_resize_grad")
    a.check()
    return grad.view.reshape(t["img"].shape)


@pytest.mark.parametrize("name", list(rc.CROP_CASES))
def test_crop_and_resize_forward(name):
    d, t, r = rc.dims(name), rc.make_inputs(name, True), rc.reference(name, True)
    got = run_forward(name, t)
    assert torch.equal(got, run_forward(name, t)), "two calls differ"
    want = dev64(DEV, r["out"].copy())
    within(got, want, torch.full((), r["fwd_bound"], dtype=torch.float64, device="cuda"), "hf_crop_and_resize." + name, "round")
    if not d["n"]:
        return
    out_of_range = torch.from_numpy(~r["ok"]).cuda()
    assert bool((got[out_of_range] == d["extrap"]).all())
    # the row that is not finite, box_ind -1, box_ind b: the extrapolation value and nothing else
    assert not np.isfinite(t["boxes"][0]).all() and t["ind"][-2] == -1 and t["ind"][-1] == d["b"]
    for row in (0, -2, -1):
        assert bool((got[row] == d["extrap"]).all())
    if d["c"] % 4 == 0:
        # images and outputs off the 16-byte boundary take the scalar-channel kernel: the same expressions, the same bits
        assert torch.equal(got, run_forward(name, t, off=True)), "the scalar-channel kernel differs"


@pytest.mark.parametrize("name", list(rc.CROP_CASES))
def test_crop_and_resize_gradient(name):
    t, r = rc.make_inputs(name, True), rc.reference(name, True)
    want, bound = dev64(DEV, r["grad"].copy()), dev64(DEV, r["grad_bound"].copy())
    never = torch.from_numpy(np.broadcast_to((r["k"] == 0)[..., None], r["grad"].shape).copy()).cuda()
    for off in (False, True):           # the second call on a map one float past a 16-byte boundary: the zero fill's head and tail
        got = run_backward(name, t, off)
        assert bool(torch.isfinite(got).all())
        within(got, want, bound, "hf_crop_and_resize_grad." + name, "round")
        assert bool((got[never] == 0.0).all())


def test_crop_and_resize_gradient_ignores_the_rows_that_fail():
    """the gradient of the whole map equals the reference computed WITHOUT the row that is not finite and the two bad box_ind rows"""
    name = "vec_c32"
    t = rc.make_inputs(name, True)
    keep = rc.finite_rows(t["boxes"]) & (t["ind"] >= 0) & (t["ind"] < rc.dims(name)["b"])
    assert (~keep).sum() == 3
    want, bound, _ = rc.ref_backward(t["img"].shape, t["boxes"][keep], t["ind"][keep], t["go"][keep])
    got = run_backward(name, t)
    assert bool(torch.isfinite(got).all())
    within(got, dev64(DEV, want), dev64(DEV, bound), "hf_crop_and_resize_grad.%s without the failing rows" % name, "round")


def run_boxes(boxes, calib, which=(True, True, True)):
    _lib, L = abi()
    b, n, _ = boxes.shape
    a = Arena(DEV)
    bx, cal = inp(boxes), inp(calib)
    outs = [Out(a, b * n * 4, passed=w) for w in which]
    h, w = rc.IMAGE_HW
    call(L.hf_roi_image_boxes(b, n, h, w, bx.p, cal.p, outs[0].p, outs[1].p, outs[2].p, _lib.stream_ptr()), "hf_roi_image_boxes")
    a.check()
    for o in outs:
        if not o.passed:
            assert bool((o.view == 12345.0).all()), "an output that was not asked for was written"
    return [o.view.reshape(b * n, 4) for o in outs]


@pytest.mark.parametrize("name", list(rc.BOX_CASES))
def test_roi_image_boxes(name):
    boxes, calib = rc.make_boxes3d(name)
    px, norm, yxyx = run_boxes(boxes, calib)
    again = run_boxes(boxes, calib)
    for g, g2 in zip((px, norm, yxyx), again):
        assert torch.equal(g, g2), "two calls differ"
    want_px, want_norm = rc.ref_boxes(boxes, calib, rc.IMAGE_HW)
    np.testing.assert_allclose(px.cpu().numpy(), want_px, **rc.PX_TOL)
    np.testing.assert_allclose(norm.cpu().numpy(), want_norm, **rc.NORM_TOL)
    assert torch.equal(yxyx, norm[:, [1, 0, 3, 2]])
    # each output alone: the same bits, the others untouched
    for i in range(3):
        only = run_boxes(boxes, calib, tuple(j == i for j in range(3)))
        assert torch.equal(only[i], (px, norm, yxyx)[i])
