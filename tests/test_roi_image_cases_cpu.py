"""CPU checks of tests/roi_image_cases.py and of the argument checks of the RoI image entry points (no GPU needed): the NumPy
restatement agrees with fusion.image_crop_and_resize on host tensors within the bounds of the table (forward on all rows, backward on
the finite rows: the tensor form's gradient of a row that is not finite is NaN), the table meets its own conditions, and
hf_roi_image_boxes / hf_crop_and_resize / hf_crop_and_resize_grad reject bad arguments before any GPU call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roi_image_cases as rc  # noqa: E402

from heterofusionrcnn_amd import fusion  # noqa: E402

NONEMPTY = tuple(k for k in rc.CROP_CASES if rc.dims(k)["n"])


def ratio(got, want, bound, name):
    diff = np.abs(got.astype(np.float64) - want)
    worst = float((diff / np.maximum(bound, 1e-300)).max()) if diff.size else 0.0
    print("%s: max |got - ref| / bound = %.3g" % (name, worst))
    assert bool((diff <= bound).all()), "%s: %d of %d elements outside the bound, worst ratio %.3g" % (name, int((diff > bound).sum()), diff.size, worst)


@pytest.mark.parametrize("name", rc.SQUARE)
def test_restatement_agrees_with_the_tensor_form_on_the_host(name):
    d, t, r = rc.dims(name), rc.make_inputs(name), rc.reference(name)
    img = torch.from_numpy(t["img"].copy())
    got = fusion.image_crop_and_resize(img, torch.from_numpy(t["boxes"].copy()), torch.from_numpy(t["ind"].copy()), d["ch"], d["extrap"])
    assert got.shape == r["out"].shape
    ratio(got.numpy(), r["out"], r["fwd_bound"], name + " forward")
    assert np.array_equal(got.numpy()[~r["ok"]], np.full_like(got.numpy()[~r["ok"]], d["extrap"]))
    # backward: the finite rows
    keep = rc.finite_rows(t["boxes"])
    assert d["n"] == 0 or not keep.all()
    boxes, ind, go = t["boxes"][keep], t["ind"][keep], t["go"][keep]
    img.requires_grad_(True)
    out = fusion.image_crop_and_resize(img, torch.from_numpy(boxes), torch.from_numpy(ind), d["ch"], d["extrap"])
    out.backward(torch.from_numpy(go))
    want, bound, k = rc.ref_backward(t["img"].shape, boxes, ind, go)
    ratio(img.grad.numpy(), want, bound, name + " backward")
    assert bool((img.grad.numpy()[k == 0] == 0.0).all())
    # a row that is not finite is out of range everywhere: the reference of all rows is the reference of the finite rows
    assert np.array_equal(want, r["grad"]) and np.array_equal(bound, r["grad_bound"])


def test_tensor_form_gradient_of_a_row_that_is_not_finite_is_nan():
    """the defect the kernels do not share: recorded here so that the host form's limit is known"""
    t = rc.make_inputs("scalar_c3")
    img = torch.from_numpy(t["img"].copy()).requires_grad_(True)
    fusion.image_crop_and_resize(img, torch.from_numpy(t["boxes"].copy()), torch.from_numpy(t["ind"].copy()), 4).sum().backward()
    assert not bool(torch.isfinite(img.grad).all())


@pytest.mark.parametrize("name", NONEMPTY)
def test_table_conditions(name):
    d, t, r = rc.dims(name), rc.make_inputs(name), rc.reference(name)
    share = 1.0 - r["ok"].mean()
    print("%s: extrapolated share %.3f, max k %d, grid rounds %s" % (name, share, r["k"].max(), rc.grid_rounds(name)))
    assert 0.1 <= share <= 0.5
    assert r["k"].max() >= 2
    assert not r["ok"][0].any() and not np.isfinite(t["boxes"][0]).all()            # the row that is not finite
    s = rc.samples(d["b"], d["h"], d["w"], d["ch"], d["cw"], t["boxes"], t["ind"])
    on_y = (s["y0"] == s["yb"])[:, :, None] & r["ok"]
    assert on_y.any()                                                               # floor == ceil is met
    # the rows with a bad box index are all extrapolation and leave the gradient alone
    tb, rb = rc.make_inputs(name, True), rc.reference(name, True)
    assert tb["ind"][-2] == -1 and tb["ind"][-1] == d["b"] and not rb["ok"][-2:].any()
    assert np.array_equal(rb["grad"], rc.ref_backward(t["img"].shape, t["boxes"], t["ind"], tb["go"][:-2])[0])


def test_table_covers_what_it_claims():
    assert rc.grid_rounds("many_c32") == (1, 1) and rc.grid_rounds("rounds_c32") == (2, 5)
    assert rc.reference("many_c32")["k"].max() >= 60
    assert rc.dims("rect_c8")["ch"] != rc.dims("rect_c8")["cw"] and rc.dims("one_pixel")["h"] == 1 and rc.dims("crop1_c5")["ch"] == 1
    assert sorted(rc.dims(k)["c"] % 4 == 0 for k in NONEMPTY).count(False) == 2
    assert [rc.dims(k)["extrap"] for k in rc.CROP_CASES].count(-3.5) == 1
    assert rc.reference("empty")["out"].shape == (0, 7, 7, 4) and not rc.reference("empty")["grad"].any()


def test_box_reference_agrees_with_the_tensor_form_on_the_host():
    for name, (b, n) in rc.BOX_CASES.items():
        boxes, calib = rc.make_boxes3d(name)
        assert b < 2 or not np.array_equal(calib[0], calib[1])
        px, norm = rc.ref_boxes(boxes, calib, rc.IMAGE_HW)
        got_px, got_norm = fusion.project_boxes_to_image(torch.from_numpy(boxes.copy()), torch.from_numpy(calib.copy()), rc.IMAGE_HW)
        np.testing.assert_allclose(got_px.numpy().reshape(-1, 4), px, **rc.PX_TOL)
        np.testing.assert_allclose(got_norm.numpy().reshape(-1, 4), norm, **rc.NORM_TOL)
        got = fusion.roi_image_boxes(torch.from_numpy(boxes.copy()), torch.from_numpy(calib.copy()), rc.IMAGE_HW)
        assert got.shape == (b * n, 4) and torch.equal(got, got_norm.reshape(-1, 4)[:, [1, 0, 3, 2]])


def test_roi_image_entry_points_reject_bad_arguments_without_a_gpu():
    """HF_EINVAL before any HIP call (fake non-null pointers, never dereferenced); empty calls are accepted"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(256)
    EINVAL, OK = _lib.HF_EINVAL, _lib.HF_OK
    # hf_roi_image_boxes(b, n, h, w, boxes3d, calib, box_px, box_norm, box_yxyx, stream)
    for b, n, h, w in ((-1, 4, 8, 8), (1, -4, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (1 << 16, 1 << 16, 8, 8), (1 << 14, 1 << 14, 8, 8)):
        assert L.hf_roi_image_boxes(b, n, h, w, one, one, one, one, one, None) == EINVAL, (b, n, h, w)
    assert L.hf_roi_image_boxes(1, 4, 8, 8, None, one, one, one, one, None) == EINVAL
    assert L.hf_roi_image_boxes(1, 4, 8, 8, one, None, one, one, one, None) == EINVAL
    assert L.hf_roi_image_boxes(0, 4, 8, 8, None, None, None, None, None, None) == OK
    assert L.hf_roi_image_boxes(2, 0, 8, 8, None, None, None, None, None, None) == OK
    assert L.hf_roi_image_boxes(1, 4, 8, 8, one, one, None, None, None, None) == OK          # no output asked for: nothing to do
    # hf_crop_and_resize(b, h, w, c, n, crop_h, crop_w, img, boxes, box_ind, extrapolation, out, stream)
    good = dict(b=2, h=8, w=8, c=4, n=3, ch=7, cw=7)
    bad = [dict(b=-1), dict(n=-1), dict(h=0), dict(w=0), dict(c=0), dict(ch=0), dict(cw=0), dict(h=-3), dict(c=-4),
           dict(b=1 << 30, h=1 << 30, w=1 << 30, c=8),                  # b h w c leaves long long
           dict(b=1 << 20, h=1 << 20, w=1 << 20, c=2),                  # 2^61 elements: their bytes leave long long
           dict(n=1 << 62, ch=2), dict(n=1 << 40, ch=1 << 20, cw=8)]
    for change in bad:
        a = dict(good, **change)
        dims = (a["b"], a["h"], a["w"], a["c"], a["n"], a["ch"], a["cw"])
        assert L.hf_crop_and_resize(*dims, one, one, one, 0.0, one, None) == EINVAL, change
        assert L.hf_crop_and_resize_grad(*dims, one, one, one, one, None) == EINVAL, change
    dims = tuple(good[k] for k in ("b", "h", "w", "c", "n", "ch", "cw"))
    for missing in range(4):
        p = [one] * 4
        p[missing] = None
        assert L.hf_crop_and_resize(*dims, p[0], p[1], p[2], 0.0, p[3], None) == EINVAL, missing
        assert L.hf_crop_and_resize_grad(*dims, p[0], p[1], p[2], p[3], None) == EINVAL, missing
    empty_n = (2, 8, 8, 4, 0, 7, 7)
    empty_b = (0, 8, 8, 4, 3, 7, 7)
    assert L.hf_crop_and_resize(*empty_n, None, None, None, 0.0, None, None) == OK
    assert L.hf_crop_and_resize(*empty_b, None, None, None, 0.0, None, None) == OK
    assert L.hf_crop_and_resize_grad(*empty_b, None, None, None, None, None) == OK
    assert L.hf_crop_and_resize_grad(*empty_n, None, None, None, None, None) == EINVAL       # a non-empty grad_img is still zero-filled
