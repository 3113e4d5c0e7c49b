"""CPU tests (-m "not gpu") of the file-to-file detector's host side: the hand-off rounding against the real text route, the
argument checks of hf_kitti_result_boxes, the row writer against write_frame_results' formatting, and the seeded cases
test_detect.py runs on the device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from heterofusionrcnn_amd import kitti_io

import detect_cases as DC


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_handoff_rounding_is_the_file_route_bit_for_bit(tmp_path):
    """round_like_handoff_file against save_proposals_and_scores -> load_proposals_and_scores -> float32, sign of zero included"""
    from heterofusionrcnn_amd.rcnn_data import round_like_handoff_file
    rng = np.random.default_rng(0)
    ties = np.arange(-64, 65, dtype=np.float32) / np.float32(16)                     # every j/16 in +-4: x.xxx5 ties among them
    edge = np.array([0.0004, -0.0004, 0.0005, -0.0005, 0.0, -0.0], dtype=np.float32)
    vals = np.concatenate([rng.uniform(-100.0, 100.0, 4000).astype(np.float32), ties, edge])
    vals = np.concatenate([vals, np.zeros((-len(vals)) % 8, np.float32)]).reshape(-1, 8)
    path = str(tmp_path / "p.txt")
    kitti_io.save_proposals_and_scores(path, vals[:, :7], vals[:, 7])
    boxes, scores = kitti_io.load_proposals_and_scores(path)
    want = np.concatenate([boxes, scores[:, None]], axis=1).astype(np.float32)
    got = round_like_handoff_file(torch.from_numpy(vals))
    assert got.dtype == torch.float32 and got.shape == vals.shape
    assert np.array_equal(_bits(got.numpy()), _bits(want))
    # the cases the proof names: a tie goes to the even thousandth, a small negative keeps its sign as zero
    one = lambda v: round_like_handoff_file(torch.tensor([v], dtype=torch.float32)).numpy()
    assert _bits(one(-0.0004))[0] == 0x80000000 and _bits(one(0.0004))[0] == 0
    assert one(0.0625)[0] == np.float32(0.062) and one(0.1875)[0] == np.float32(0.188)


def test_handoff_in_memory_uses_the_tensors_in_place():
    from heterofusionrcnn_amd.rcnn_data import handoff_in_memory
    xyz, inten = torch.zeros(1, 4, 3), torch.zeros(1, 4, 1)
    out = {"proposals": torch.tensor([[[1.23456, -0.0004, 3.0005, 4, 5, 6, 0.06251]]]), "rpn_fts": torch.zeros(1, 4, 8),
           "fg_mask": torch.zeros(1, 4, dtype=torch.bool), "proposal_scores": torch.zeros(1, 1)}
    h = handoff_in_memory(out, xyz, inten)
    assert list(h) == ["xyz", "rpn_fts", "intensity", "fg_mask", "proposals"]             # RcnnModel.detect's leading arguments
    assert h["xyz"] is xyz and h["intensity"] is inten and h["rpn_fts"] is out["rpn_fts"] and h["fg_mask"] is out["fg_mask"]
    assert h["proposals"] is out["proposals"]
    r = handoff_in_memory(out, xyz, inten, handoff_rounding=True)
    assert r["rpn_fts"] is out["rpn_fts"] and r["proposals"] is not out["proposals"]
    assert r["proposals"][0, 0].tolist() == [np.float32(v).item() for v in (1.235, -0.0, 3.0, 4, 5, 6, 0.063)]


def test_result_boxes_entry_point_rejects_bad_arguments_without_a_gpu():
    """HF_EINVAL before any HIP call; an empty problem launches nothing"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    args = lambda b, n, ptrs: L.hf_kitti_result_boxes(b, n, *ptrs[:5], 0.1, *ptrs[5:], None)
    ok = [one] * 7
    assert args(0, 4, ok) == _lib.HF_EINVAL
    assert args(-1, 4, ok) == _lib.HF_EINVAL
    assert args(0, 0, ok) == _lib.HF_EINVAL
    assert args(3, -1, ok) == _lib.HF_EINVAL
    for k in range(7):                                                                    # each pointer in turn
        assert args(3, 4, ok[:k] + [None] + ok[k + 1:]) == _lib.HF_EINVAL, k
    assert args(3, 0, ok) == _lib.HF_OK
    assert args(3, 0, [None] * 7) == _lib.HF_OK


def test_row_writer_formats_as_write_frame_results(tmp_path):
    """write_result_rows on rows holding the host's own rectangles writes the bytes write_frame_results writes"""
    from heterofusionrcnn_amd.inference import RESULT_ROW_COLUMNS, write_frame_results, write_result_rows
    cases = DC.make_cases()
    keep, b2, _, _, _ = DC.reference(cases)
    at = 0
    for f, det in enumerate(cases["dets"]):
        n = len(det["boxes"])
        rows = np.zeros((n, RESULT_ROW_COLUMNS))
        rows[:, 0:4] = np.nan_to_num(b2[at:at + n])
        rows[:, 4:11], rows[:, 11], rows[:, 12], rows[:, 13] = det["boxes"], det["scores"], det["classes"], keep[at:at + n]
        a, b = str(tmp_path / ("a%d.txt" % f)), str(tmp_path / ("b%d.txt" % f))
        wrote = write_frame_results(a, det, cases["p2"][f], tuple(int(v) for v in cases["wh"][f]), DC.SCORE_THRESHOLD)
        assert write_result_rows(b, rows) == wrote == int(keep[at:at + n].sum())
        assert open(a, "rb").read() == open(b, "rb").read()
        assert (wrote > 0) == (n > 0)
        at += n


def test_generated_cases_vary_p2_and_image_size_among_the_frames_with_rows():
    """a kernel that read another frame's P2 or image size must not pass: rows under at least two sizes in each call, under both
    P2 matrices the committed calib files offer in one, and under every frame's size across the calls"""
    p2 = DC.frames_p2()
    assert len({p.tobytes() for p in p2}) == 2 and len(set(DC.SIZES)) == 3          # the goldens hold two distinct P2
    sizes_seen, p2_seen = set(), []
    for empty in DC.EMPTY_FRAMES:
        cases = DC.make_cases(empty)
        live = [f for f, d in enumerate(cases["dets"]) if len(d["boxes"])]
        assert live == [f for f in range(3) if f != empty]
        sizes = {tuple(int(v) for v in cases["wh"][f]) for f in live}
        assert len(sizes) >= 2
        sizes_seen |= sizes
        p2_seen.append(len({cases["p2"][f].tobytes() for f in live}))
    assert sizes_seen == set(DC.SIZES) and max(p2_seen) == 2
    # and they matter: with the two live frames' sizes exchanged keep decisions change, in both calls; with their P2 exchanged
    # (the call whose live frames have different ones) kept rectangles move by far more than the test's tolerance
    for empty in DC.EMPTY_FRAMES:
        cases = DC.make_cases(empty)
        a, b = [f for f in range(3) if f != empty]
        swap = np.arange(3)
        swap[[a, b]] = [b, a]
        keep, b2 = DC.reference(cases)[:2]
        assert (DC.reference(dict(cases, wh=cases["wh"][swap]))[0] != keep).sum() >= 10
    cases = DC.make_cases(1)
    keep, b2 = DC.reference(cases)[:2]
    keep_p, b2_p = DC.reference(dict(cases, p2=cases["p2"][[2, 1, 0]]))[:2]
    both = keep & keep_p
    assert both.sum() >= 20 and np.abs(b2[both] - b2_p[both]).max() > 1.0


@pytest.mark.parametrize("empty", DC.EMPTY_FRAMES)
def test_generated_cases_cover_every_branch_and_stay_under_the_cap(empty):
    cases = DC.make_cases(empty)
    keep, b2, near, score_ok, projected = DC.reference(cases)
    n = len(keep)
    assert 150 <= n <= 250 and len(cases["dets"][empty]["boxes"]) == 0
    assert near.sum() <= DC.CAP * n, "too many rows sit on a decision boundary: change the seed"
    kinds = np.array(cases["kinds"])
    raw = np.concatenate([[DC.raw_rectangle(bx, cases["p2"][f]) for bx in det["boxes"]] for f, det in enumerate(cases["dets"])
                          if len(det["boxes"])])
    wh = np.concatenate([np.tile(cases["wh"][f], (len(det["boxes"]), 1)) for f, det in enumerate(cases["dets"])])
    iw, ih = wh[:, 0], wh[:, 1]
    is_ = lambda k: kinds == k
    assert projected[is_("inside")].all() and (raw[is_("inside"), 0] > 0).all() and (raw[is_("inside"), 2] < iw[is_("inside")]).all()
    assert projected[is_("cut_left")].all() and (raw[is_("cut_left"), 0] < 0).all()
    assert projected[is_("cut_right")].all() and (raw[is_("cut_right"), 2] > iw[is_("cut_right")]).all()
    assert projected[is_("cut_top")].all() and (raw[is_("cut_top"), 1] < 0).all()
    assert projected[is_("cut_bottom")].all() and (raw[is_("cut_bottom"), 3] > ih[is_("cut_bottom")]).all()
    assert (raw[is_("out_left"), 2] < 0).all() and (raw[is_("out_right"), 0] > iw[is_("out_right")]).all()
    assert (raw[is_("out_top"), 3] < 0).all() and (raw[is_("out_bottom"), 1] > ih[is_("out_bottom")]).all()
    for k in ("out_left", "out_right", "out_top", "out_bottom", "wide", "tall"):
        assert not projected[is_(k)].any(), k
    w_, h_ = raw[:, 2] - raw[:, 0], raw[:, 3] - raw[:, 1]
    assert (w_[is_("wide")] > 0.8 * iw[is_("wide")]).all() and (h_[is_("wide")] <= 0.8 * ih[is_("wide")]).all()
    assert (h_[is_("tall")] > 0.8 * ih[is_("tall")]).all() and (w_[is_("tall")] <= 0.8 * iw[is_("tall")]).all()
    behind = np.concatenate([det["boxes"] for det in cases["dets"]])[is_("behind")]
    reach = 0.5 * (np.abs(np.sin(behind[:, 6])) * behind[:, 3] + np.abs(np.cos(behind[:, 6])) * behind[:, 4])
    assert (behind[:, 2] - reach < 0).all() and (behind[:, 2] + reach > 0).all()
    # scores below, exactly at and above the threshold, among rows the projector accepts
    t = np.float32(round(DC.SCORE_THRESHOLD, 3))
    scores = np.concatenate([det["scores"] for det in cases["dets"]])
    for s, ok in ((np.nextafter(t, np.float32(0)), False), (t, True), (np.nextafter(t, np.float32(1)), True)):
        sel = (scores == s) & projected
        assert sel.sum() >= 5 and (keep[sel] == ok).all() and (score_ok[scores == s] == ok).all()
    assert 30 <= keep.sum() <= n - 30
