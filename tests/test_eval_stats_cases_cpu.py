"""CPU tests of tests/eval_stats_cases.py and of the argument checks of hf_proposal_stats / hf_argmax_accuracy (no GPU: the checks
return before anything is launched)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_stats_cases as ec  # noqa: E402
from abi_harness import abi  # noqa: E402


def test_the_cases_cover_what_the_kernels_branch_on():
    pc = ec.PROPOSAL_CASES
    assert {c["b"] for c in pc} >= {1, 3}
    assert {c["m"] for c in pc} >= {1, 63, 64, 65, 100, 512}
    assert {c["g"] for c in pc} >= {0, 1, 3, 128}
    assert any(fr["n"] < c["m"] for c in pc for fr in c["frames"]), "no proposal_count < m"
    assert any(0 < fr["ng"] < c["g"] for c in pc for fr in c["frames"]), "no gt_count < g"
    assert any(any(fr["ng"] == 0 for fr in c["frames"]) and any(fr["ng"] > 0 for fr in c["frames"]) for c in pc), \
        "no frame without labels next to frames with labels"
    assert any(fr["twin_gt"] and fr["ng"] >= 2 for c in pc for fr in c["frames"])
    assert any(fr["twin_roi"] and fr["n"] >= 2 for c in pc for fr in c["frames"])
    ac = ec.ACCURACY_CASES
    assert {a[0] for a in ac} >= {1, 63, 64, 65, 257, 16384} and {a[1] for a in ac} >= {1, 3} and {a[2] for a in ac} >= {2, 4, 8}


@pytest.mark.parametrize("c", ec.PROPOSAL_CASES, ids=ec.case_id)
def test_proposal_case_conditions(c):
    t = ec.make_proposal_inputs(c)
    recalls = ec.check_proposal_case(c, t["mats"])           # raises when a margin or the ordered-recall condition fails
    assert recalls == t["recalls"]
    for fr, iou, (labels, r50, r70) in zip(c["frames"], t["mats"], recalls):
        assert iou.shape == (fr["n"], fr["ng"]) and labels == fr["ng"]
        if iou.size:
            col = iou.max(axis=0)
            assert np.abs(col - 0.5).min() >= ec.MARGIN and np.abs(col - 0.7).min() >= ec.MARGIN
    if ec.can_hold_ordered_recalls(c):
        assert any(0 < r70 < r50 < labels for labels, r50, r70 in recalls), recalls
    else:
        assert c["m"] < 3 or c["g"] < 3
    if any(fr["ng"] for fr in c["frames"]) and c["m"] >= 3:
        assert any(r50 > 0 for _, r50, _ in recalls), "nothing is recalled at all"
    # an all-zero row among the valid proposals of a frame with labels (best_gt 0), twins where asked for
    for fr, iou, f in zip(c["frames"], t["mats"], range(c["b"])):
        if fr["ng"] and fr["n"] > fr["r70"] + fr["r50"]:
            assert (iou.max(axis=1) == 0).any(), "no proposal far from every GT"
        if fr["twin_gt"] and fr["ng"] >= 2:
            assert np.array_equal(t["gt"][f, 0], t["gt"][f, 1]) and (iou[:, 0] > 0).any(), "no proposal on the twin GT"
        if fr["twin_roi"] and fr["n"] >= 2:
            p = t["proposals"][f, :fr["n"]]
            assert any(np.array_equal(p[i], p[(i + 1) % fr["n"]]) for i in range(fr["n"]))


def test_restatement_on_a_hand_made_example():
    """box_util.compute_recall_iou's definitions on 3 proposals x 2 labels, written out"""
    iou3 = np.array([[[0.80, 0.10], [0.00, 0.00], [0.60, 0.60]]], np.float32)
    iou2 = np.array([[[0.90, 0.20], [0.95, 0.00], [0.70, 0.75]]], np.float32)
    props = np.zeros((1, 3, 7), np.float32)
    gt = np.zeros((1, 2, 8), np.float32)
    props[0, :, 6] = [0.5, -1.0, 2.0]
    gt[0, :, 6] = [0.25, 3.0]
    b3, b2, bg, counts, sums, mags = ec.ref_proposal_stats(iou3, iou2, props, np.array([3], np.int32), gt, np.array([2], np.int32))
    assert b3.tolist() == [[np.float32(0.80), 0.0, np.float32(0.60)]]
    assert b2.tolist() == [[np.float32(0.90), np.float32(0.95), np.float32(0.75)]]
    assert bg.tolist() == [[0, 0, 0]]                     # all-zero row -> 0; equal maxima -> the first
    # column maxima 0.80 and 0.60: both > 0.5, one > 0.7
    assert counts.tolist() == [[3, 2, 2, 1]]
    f32 = np.float32
    want = [float(f32(0.90)) + float(f32(0.95)) + float(f32(0.75)), float(f32(0.80)) + float(f32(0.60)),
            float(f32(0.25)) + float(f32(1.25)) + float(f32(1.75))]
    assert np.allclose(sums[0], want, rtol=1e-15, atol=0) and np.allclose(mags[0], want, rtol=1e-15, atol=0)
    # strictness: a column maximum of exactly 0.5 is not recalled at 0.5 (0.75 is exact in fp32 too: recalled at both)
    edge = np.array([[[0.5, 0.75]]], np.float32)
    _, _, _, counts, _, _ = ec.ref_proposal_stats(edge, edge, props[:, :1], np.array([1], np.int32), gt, np.array([2], np.int32))
    assert counts.tolist() == [[1, 2, 1, 1]]
    # short counts, a frame without labels
    _, _, bg, counts, sums, _ = ec.ref_proposal_stats(iou3, iou2, props, np.array([2], np.int32), gt, np.array([0], np.int32))
    assert bg.tolist() == [[-1, -1, -1]] and counts.tolist() == [[2, 0, 0, 0]] and sums.tolist() == [[0.0, 0.0, 0.0]]


def test_accuracy_restatement_and_cases():
    logits = np.array([[1, 1], [0, 2], [3, 3], [2, 1]], np.float32)
    target = np.array([0, 1, -1, 1], np.int32)
    assert ec.ref_argmax_accuracy(logits, target, 1).tolist() == [3]
    assert ec.ref_argmax_accuracy(logits, target, 2).tolist() == [2, 1]
    for case in ec.ACCURACY_CASES:
        rpg, groups, c = case
        lg, tg = ec.make_accuracy_inputs(case)
        assert lg.shape == (rpg * groups, c) and tg.min() >= -1 and tg.max() <= c - 1
        srt = np.sort(lg, axis=1)
        if rpg >= 63:
            assert (srt[:, -1] == srt[:, -2]).any(), "no row with equal maxima"
            assert (tg == -1).any()
        if groups == 3:
            got = ec.ref_argmax_accuracy(lg, tg, 3)
            assert got[0] == rpg and got[1] == 0


def test_proposal_stats_rejects_arguments_outside_the_limits():
    _lib, L = abi()
    one = ctypes.c_void_p(256)                # never dereferenced: the checks come first
    call = lambda b, m, g: L.hf_proposal_stats(b, m, g, one, one, one, one, None, None, one, one, one, one, one, one, 1 << 40, None)
    for b, m, g in ((-1, 1, 1), (ec.MAX_B + 1, 1, 1), (1, 0, 1), (1, -3, 1), (1, ec.MAX_M + 1, 1), (1, 1, -1), (1, 1, ec.MAX_G + 1)):
        assert call(b, m, g) == _lib.HF_EINVAL, (b, m, g)
        assert L.hf_proposal_stats_workspace(b, m, g) == 0, (b, m, g)
    pad = lambda v: (v + 255) & ~255
    assert L.hf_proposal_stats_workspace(8, 100, 16) == 2 * pad(4 * 8 * 100 * 16)
    assert L.hf_proposal_stats_workspace(ec.MAX_B, ec.MAX_M, ec.MAX_G) == 2 * 4 * ec.MAX_B * ec.MAX_M * ec.MAX_G
    assert L.hf_proposal_stats_workspace(3, 64, 0) == 0
    assert call(0, 1, 1) == _lib.HF_OK        # nothing to do, nothing launched
    # missing arrays and a workspace that is too small
    assert L.hf_proposal_stats(1, 1, 1, None, one, one, one, None, None, one, one, one, one, one, one, 1 << 40, None) == _lib.HF_EINVAL
    assert L.hf_proposal_stats(1, 1, 1, one, one, None, one, None, None, one, one, one, one, one, one, 1 << 40, None) == _lib.HF_EINVAL
    assert L.hf_proposal_stats(1, 1, 1, one, one, one, one, None, None, one, one, one, one, None, one, 1 << 40, None) == _lib.HF_EINVAL
    assert L.hf_proposal_stats(1, 1, 1, one, one, one, one, None, None, one, one, one, one, one, one, 511, None) == _lib.HF_EWORKSPACE


def test_argmax_accuracy_rejects_arguments_outside_the_limits():
    _lib, L = abi()
    one = ctypes.c_void_p(256)
    for rows, c, groups in ((8, 1, 1), (8, 9, 1), (8, 0, 1), (8, 4, 0), (8, 4, -1), (8, 4, 3), (-4, 4, 1)):
        assert L.hf_argmax_accuracy(rows, c, groups, one, one, one, None) == _lib.HF_EINVAL, (rows, c, groups)
    assert L.hf_argmax_accuracy(8, 4, 2, None, one, one, None) == _lib.HF_EINVAL
    assert L.hf_argmax_accuracy(8, 4, 2, one, one, None, None) == _lib.HF_EINVAL
