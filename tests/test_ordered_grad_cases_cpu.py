"""CPU checks of tests/ordered_grad_cases.py and of the argument checks of the ordered image-gradient entries (no GPU needed):
the sequential reference equals np.add.at on a float32 array bit for bit; in the cases named order-sensitive, adding in descending order
changes the bits of at least one pixel with three or more entries and of no pixel with at most two; the table holds what it claims;
hf_project_gather_grad_ordered / hf_crop_and_resize_grad_ordered return HF_EINVAL for bad arguments before any GPU call and their
workspace functions return sizes from shapes alone."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ordered_grad_cases as oc  # noqa: E402
import roi_image_cases as rc  # noqa: E402

PROJECT = tuple(oc.PROJECT_CASES)
CROP = tuple(rc.CROP_CASES)
ORDER_SENSITIVE_PROJECT = ("scalar_c3", "step64_c32", "chunk1024_c4", "straddle_c5", "wide_c40", "global_sort_c2")
ORDER_SENSITIVE_CROP = ("scalar_c3", "vec_c32", "many_c32", "tiny", "one_pixel", "rect_c8", "rounds_c32")    # crop1_c5 is not: exempt


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def entries(kind, name):
    if kind == "project":
        return oc.entries_project(name)
    t = rc.make_inputs(name, True)
    return oc.entries_crop(t["img"].shape, t["boxes"], t["ind"], t["go"])


ALL = [("project", n) for n in PROJECT] + [("crop", n) for n in CROP]


@pytest.mark.parametrize("kind,name", ALL)
def test_reference_is_add_at_in_float32(kind, name):
    targets, valid, key, term = entries(kind, name)
    want = np.zeros((targets, term.shape[1]), np.float32)
    np.add.at(want, key[valid], term[valid])
    ref = oc.sequential(targets, valid, key, term)
    assert ref.dtype == np.float32 and np.array_equal(bits(ref), bits(want))
    cached = oc.project_reference(name) if kind == "project" else oc.crop_reference(name, True)
    assert np.array_equal(bits(cached["grad"]).reshape(-1), bits(ref).reshape(-1))
    assert np.array_equal(cached["k"].reshape(-1), oc.counts(targets, valid, key))
    assert not np.signbit(ref[oc.counts(targets, valid, key) == 0]).any()             # a target that nothing names is +0


@pytest.mark.parametrize("kind,name", ALL)
def test_order_shows_in_the_bits_only_from_three_entries(kind, name):
    targets, valid, key, term = entries(kind, name)
    k = oc.counts(targets, valid, key)
    up, down = oc.sequential(targets, valid, key, term), oc.sequential(targets, valid, key, term, descending=True)
    moved = (bits(up) != bits(down)).any(axis=1)
    print("%s %s: %d entries, %d pixels with >= 3 entries, %d of them change with the order, longest list %d"
          % (kind, name, int(valid.sum()), int((k >= 3).sum()), int(moved.sum()), int(k.max()) if k.size else 0))
    assert not moved[k <= 2].any()
    if name in (ORDER_SENSITIVE_PROJECT if kind == "project" else ORDER_SENSITIVE_CROP):
        assert (k >= 3).any() and moved[k >= 3].any()


def test_crop_terms_are_those_of_the_fp64_reference():
    """the fp32 terms and keys restate what roi_image_cases.ref_backward scatters: same counts, and the sum within its bound"""
    for name in CROP:
        t, r = rc.make_inputs(name, True), rc.reference(name, True)
        got = oc.crop_reference(name, True)
        assert np.array_equal(got["k"], r["k"])
        assert bool((np.abs(got["grad"].astype(np.float64) - r["grad"]) <= r["grad_bound"]).all())
        assert got["grad"].shape == t["img"].shape


def test_table_covers_what_it_claims():
    k = {n: oc.project_reference(n)["k"] for n in PROJECT}
    assert 17 <= k["scalar_c3"].max() <= 24 and (k["scalar_c3"] <= 16).any()         # both sides of the 16 a thread sorts alone
    assert k["step64_c32"].max() == 70 and k["chunk1024_c4"].max() == 1300 and k["global_sort_c2"].max() == 5000 > 4096
    b, p, h, w, c = oc.PROJECT_CASES["straddle_c5"]
    flat = k["straddle_c5"].reshape(-1)
    hot = [t for f in oc.HOT_PIXELS.values() for t in f]
    assert len(hot) == 10 and all(flat[t] >= 17 for t in hot) and all(min(t % 1024, 1024 - t % 1024) <= 1 for t in hot)
    assert not k["straddle_c5"][oc.ZERO_FRAME].any() and b * h * w > 4 * 4096
    pix = oc.make_project("straddle_c5")["pix"]
    assert (pix[..., 0] == -1).any() and (pix[..., 0] == w).any() and (pix[..., 1] == -1).any() and (pix[..., 1] == h).any()
    assert oc.PROJECT_CASES["wide_c40"][4] > 32 and oc.PROJECT_CASES["wide_c40"][4] & (oc.PROJECT_CASES["wide_c40"][4] - 1)
    for n in PROJECT:
        go = oc.make_project(n)["go"]
        if go.size:
            mag = np.abs(go[go != 0])
            assert (np.signbit(go) & (go == 0)).any() and mag.min() >= 2.0 ** -12 and mag.max() < 2.0 ** 13
    assert oc.project_reference("empty_p")["grad"].shape == (2, 4, 6, 4) and not oc.project_reference("empty_p")["grad"].any()
    assert oc.project_reference("empty_b")["grad"].size == 0


def test_levels_of_the_crop_table_meet_two_taps_on_one_pixel():
    """floor == ceil: two taps of one sample are two entries of one pixel, in tap order"""
    t = rc.make_inputs("tiny", True)
    targets, valid, key, term = oc.entries_crop(t["img"].shape, t["boxes"], t["ind"], t["go"])
    key4, valid4 = key.reshape(-1, 4), valid.reshape(-1, 4)
    assert (valid4[:, 0] & (key4[:, 0] == key4[:, 1])).any() and (valid4[:, 0] & (key4[:, 0] == key4[:, 2])).any()


def test_ordered_entries_reject_bad_arguments_without_a_gpu():
    """HF_EINVAL before any HIP call (fake non-null pointers, never dereferenced); b == 0 is accepted; sizes from shapes alone"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one, ws = ctypes.c_void_p(256), ctypes.c_void_p(4096)
    EINVAL, OK = _lib.HF_EINVAL, _lib.HF_OK
    big = 1 << 40
    # hf_project_gather_grad_ordered(b, p, h, w, c, grad_out, pix, grad_img, ws, ws_bytes, stream)
    good = dict(b=2, p=100, h=8, w=8, c=4)
    order = ("b", "p", "h", "w", "c")
    for change in (dict(b=-1), dict(p=-1), dict(h=0), dict(w=0), dict(c=0), dict(h=-3), dict(b=1 << 11, h=1 << 10, w=1 << 10),
                   dict(b=1 << 16, h=1 << 16), dict(b=1 << 16, p=1 << 15)):
        a = dict(good, **change)
        dims = tuple(a[k] for k in order)
        assert L.hf_project_gather_grad_ordered(*dims, one, one, one, ws, big, None) == EINVAL, change
        assert L.hf_project_gather_grad_ordered_workspace(*dims) == 0, change
    dims = tuple(good[k] for k in order)
    need = L.hf_project_gather_grad_ordered_workspace(*dims)
    assert need % 16 == 0 and need >= 4 * (2 * 8 * 8 + 2 * 200)              # a count per pixel, a key and a slot per entry
    for missing in range(4):
        p = [one, one, one, ws]
        p[missing] = None
        assert L.hf_project_gather_grad_ordered(*dims, *p, big, None) == EINVAL, missing
    assert L.hf_project_gather_grad_ordered(*dims, one, one, one, ws, need - 1, None) == EINVAL
    assert L.hf_project_gather_grad_ordered(*dims, one, one, one, ctypes.c_void_p(4100), big, None) == EINVAL     # not 16-byte aligned
    assert L.hf_project_gather_grad_ordered(0, 100, 8, 8, 4, None, None, None, None, 0, None) == OK
    assert L.hf_project_gather_grad_ordered_workspace(0, 100, 8, 8, 4) == 0
    assert L.hf_project_gather_grad_ordered(2, 0, 8, 8, 4, None, None, None, ws, big, None) == EINVAL           # the map is still written
    assert L.hf_project_gather_grad_ordered_workspace(2, 0, 8, 8, 4) > 0
    # hf_crop_and_resize_grad_ordered(b, h, w, c, n, crop_h, crop_w, grad_out, boxes, box_ind, grad_img, ws, ws_bytes, stream)
    good = dict(b=2, h=8, w=8, c=4, n=3, ch=7, cw=7)
    order = ("b", "h", "w", "c", "n", "ch", "cw")
    for change in (dict(b=-1), dict(n=-1), dict(h=0), dict(w=0), dict(c=0), dict(ch=0), dict(cw=0), dict(c=-4),
                   dict(b=1 << 30, h=1 << 30, w=1 << 30, c=8), dict(b=1 << 11, h=1 << 10, w=1 << 10), dict(n=1 << 62, ch=2),
                   dict(n=1 << 24, ch=8, cw=4)):                                   # 2^31 entries
        a = dict(good, **change)
        dims = tuple(a[k] for k in order)
        assert L.hf_crop_and_resize_grad_ordered(*dims, one, one, one, one, ws, big, None) == EINVAL, change
        assert L.hf_crop_and_resize_grad_ordered_workspace(*dims) == 0, change
    dims = tuple(good[k] for k in order)
    need = L.hf_crop_and_resize_grad_ordered_workspace(*dims)
    assert need % 16 == 0 and need >= 4 * (2 * 8 * 8 + 2 * 3 * 49 * 4)
    for missing in range(5):
        p = [one, one, one, one, ws]
        p[missing] = None
        assert L.hf_crop_and_resize_grad_ordered(*dims, *p, big, None) == EINVAL, missing
    assert L.hf_crop_and_resize_grad_ordered(*dims, one, one, one, one, ws, need - 1, None) == EINVAL
    assert L.hf_crop_and_resize_grad_ordered(0, 8, 8, 4, 3, 7, 7, None, None, None, None, None, 0, None) == OK
    assert L.hf_crop_and_resize_grad_ordered(2, 8, 8, 4, 0, 7, 7, None, None, None, None, ws, big, None) == EINVAL
    assert L.hf_crop_and_resize_grad_ordered_workspace(2, 8, 8, 4, 0, 7, 7) > 0
