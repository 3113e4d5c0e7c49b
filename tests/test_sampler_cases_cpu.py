"""CPU tests of tests/sampler_cases.py, the case table and NumPy restatement that tests/test_sampler_abi.py holds csrc/rpn_batch.hip and
csrc/rcnn_targets.hip against: the table reaches every branch, the conditions on the inputs hold for the committed seeds, the restated
permutation is a bijection, the restated streams have the statistics the samplers promise (together with the draw-for-draw equality on
the GPU these carry over to the kernels), the fp64 IoU gives the hand answers, and the restated limits and layouts equal the library's
host entry points."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402


def chi2(counts, expected):
    return float(((np.asarray(counts, np.float64) - expected) ** 2 / expected).sum())


def chi2_band(dof):
    """mean + 6 sigma of a chi-square with dof degrees of freedom"""
    return dof + 6.0 * np.sqrt(2.0 * dof)


def binomial_band(k, prob):
    return 6.0 * np.sqrt(k * prob * (1 - prob))


def call_keys(seed, count, frame, purpose):
    return np.array([sc.rb_key(seed, k, frame, purpose) for k in range(count)], dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ the table
def test_case_ids_are_unique_and_counted():
    ids = [sc.case_id(c) for c in sc.all_cases()]
    assert len(set(ids)) == len(ids)
    count = collections.Counter(c["kind"] for c in sc.all_cases())
    # update these numbers when the table changes
    assert dict(count) == {"points": 12, "labels": 22, "image": 7, "targets": 22}
    for c in sc.all_cases():
        assert len(c["frames"]) <= 5 if "frames" in c else c["b"] <= 5
        if c["kind"] == "points":
            assert c["p"] <= 1000
        if c["kind"] == "targets":
            assert c["m"] <= 512 and c["r"] <= 512 and c["g"] <= 128


def test_points_cases_reach_every_branch():
    branches, multi_block, short_frames, p_seen, raw_seen = set(), 0, 0, set(), set()
    flips, status = set(), set()
    for c in sc.cases_of("points"):
        t = sc.make_inputs(c)
        for call in range(c["calls"]):
            xyz, inten, src, st, state, info = sc.ref_rpn_points(c, t, call)
            assert (info["writes"] == 1).all(), "an output slot of %s is written %s times" % (sc.case_id(c), np.unique(info["writes"]))
            assert (src != sc.SENT_I).all()
            branches |= set(info["branch"])
            status |= set(st.tolist())
            assert state.tolist() == [c["state"][0], c["state"][1] + call + 1]
        chunks = -(-t["max_frame"] // sc.THREADS)
        multi_block += sum(1 for k in info["blocks"] if k > 1)
        short_frames += sum(1 for k in info["blocks"] if k < chunks)
        p_seen.add(c["p"])
        raw_seen |= {f[0] for f in c["frames"]}
        flips |= {f[3] for f in c["frames"]}
        # sampled rows really are of the class the branch allows
        for f, br in enumerate(info["branch"]):
            nn, nf = info["counts"][f]
            s, e = max(int(t["offsets"][f]), 0), min(int(t["offsets"][f + 1]), t["total"])
            cls = sc.classify(t["points"][s:e], t["velo_to_rect"][f], t["p2"][f], t["wh"][f])[0]
            if br != "empty":
                got = cls[src[f]]
                assert (got != 0).all()
                if br in ("far_only", "near_none"):
                    assert (got == 2).all(), "a near point in a frame whose far points fill P"
                if br in ("mixed", "far_none"):
                    assert (got == 2).sum() == nf, "every far point exactly once"
                if br not in ("far_only", "near_none", "mixed", "far_none"):
                    assert set(src[f].tolist()) == set(np.nonzero(cls)[0].tolist()), "every kept point at least once"
    assert branches == set(sc.PLACEMENT_BRANCHES), set(sc.PLACEMENT_BRANCHES) - branches
    assert status == {0, sc.STATUS_EMPTY, sc.STATUS_TOO_MANY_FAR}
    assert multi_block > 0 and short_frames > 0 and flips == {0, 1}
    assert p_seen == {1, 2, 3, 4, 5, 16, 17, 64, 100, 256, 257, 1000}
    assert raw_seen == {0, 1, 63, 64, 65, 255, 256, 257, 513, 1000}
    assert {tuple(c["state"]) for c in sc.cases_of("points")} == {(7, 0), (-1, 2 ** 40 + 3)}
    assert any(c["calls"] == 2 for c in sc.cases_of("points")) and any(c["clamp"] for c in sc.cases_of("points"))


def test_points_view_conditions_and_boundary_points():
    on_bound = 0
    for c in sc.cases_of("points"):
        t = sc.make_inputs(c)
        for f in range(len(c["frames"])):
            s, e = max(int(t["offsets"][f]), 0), min(int(t["offsets"][f + 1]), t["total"])
            cls, rect, margin = sc.classify(t["points"][s:e], t["velo_to_rect"][f], t["p2"][f], t["wh"][f])
            assert ((margin == 0) | (margin >= sc.VIEW_MARGIN)).all()
            assert (cls[(margin == 0) & (rect[:, 2] != sc.FAR_DEPTH)] == 0).all(), "a point on a view bound is out of view"
            assert (cls[rect[:, 2] == sc.FAR_DEPTH] == 2).all(), "z == 40 is far"
            on_bound += int((margin == 0).sum())
    assert on_bound > 50


def test_labels_cases_reach_every_rule():
    total = collections.Counter()
    shapes, counts = set(), set()
    for c in sc.cases_of("labels"):
        cls, reg, info = sc.ref_rpn_labels(c)
        total.update(info)
        shapes.add((c["b"], c["p"], c["g"]))
        counts |= {n - c["g"] if n >= c["g"] and n > 0 else n for n in c["counts"]}
        assert set(np.unique(cls)) <= {-1, 0, 1, 2, 3}
        assert (reg[cls > 0] != 0).any(-1).all() and not reg[(cls == 0)].any()
    assert shapes == {(1, 1, 0), (1, 5, 1), (2, 257, 3), (1, 300, 128)}
    assert {-3, 0, 5} <= counts
    for key in ("on_face", "ring_then_inside", "inside_then_ring", "ring", "inside"):
        assert total[key] > 0, key
    assert {c["expand"] for c in sc.cases_of("labels")} == {0.0, 0.2}


def test_image_cases_reach_every_rule():
    kinds, blocks = set(), set()
    for c in sc.cases_of("image"):
        t = sc.make_inputs(c)
        image, noise, state, info = sc.ref_image(c, t)
        kinds |= set(info["kind"])
        blocks |= set(info["blocks"])
        for f, k in enumerate(info["kind"]):
            if k == "invalid":
                assert not image[f].any() and not noise[f].any()
            if "one_pixel" in k or "zero_cov" in k or not k.startswith("jitter"):
                assert not noise[f].any()
            elif k.startswith("jitter"):
                assert np.abs(noise[f]).max() > 0
    assert kinds == {"plain", "plain_flip", "jitter", "jitter_flip", "jitter_one_pixel", "jitter_flip_one_pixel", "jitter_zero_cov", "invalid"}
    assert 2 in blocks, "4097 pixels: one past the first 4096-pixel block of the sums"
    assert {(c["src"], c["out"]) for c in sc.cases_of("image")} >= {((1, 1), (3, 2)), ((5, 7), (5, 7)), ((8, 6), (16, 12)), ((6, 8), (3, 16)),
                                                                       ((64, 64), (7, 3)), ((4097, 1), (33, 1))}


def test_targets_cases_reach_every_branch_and_hold_the_conditions():
    branches, mixes, jitter, trips, shapes = set(), set(), set(), set(), set()
    dup = 0
    ties = {2: 0, 4: 0}
    for c in sc.cases_of("targets"):
        t = sc.make_inputs(c)
        shapes.add((c["b"], c["m"], c["g"], c["r"] if c["train"] else "val"))
        for f, (iou, gap, oh) in enumerate(t["mats"]):
            n, ng = iou.shape
            sc.check_iou_conditions(c, iou, gap, oh, t["proposals"][f, :n], t["gt"][f, :ng, :7])
        assert (t["proposals"][:, :, 3] > 0).all(), "padding rows hold huge boxes"
        for call in range(c["calls"]):
            ref = sc.ref_rcnn_targets(c, t, call, strict=True)
            info = ref["info"]
            assert info["closest"] >= sc.DELTA
            branches |= set(info["branch"])
            mixes |= set(info["mix"])
            jitter |= info["jitter"]
            trips |= info["second_trip"]
            dup += info["dup_fg_slots"]
        if c["train"] and c["fg_ratio"] == 0.5:
            assert sc.fg_per_image(c) == {1: 0, 3: 2, 4: 2, 5: 2, 7: 4, 64: 32, 512: 256}[c["r"]]      # half to even
    assert branches == {"fg+bg", "fg", "bg", "neither", "empty", "val", "val_empty"}
    assert mixes >= {"below", "above", "below_one", "hard+easy", "hard_only", "easy_only"}
    assert jitter >= {"method1", "method2", "method3", "kept", "moved", "fg_stopped_early", "fg_ran_out", "bg_ran_out", "bg_stopped_last",
                      "no_gt_no_try", "row0", "row1", "row2", "row3", "row4"}
    assert trips == {"roi_loop", "slot_loop"}
    assert dup > 0, "no RoI fills two fg slots"
    assert shapes >= {(1, 1, 1, 1), (2, 5, 0, 4), (3, 64, 3, 7), (2, 257, 5, 64), (1, 512, 128, 512), (4, 40, 4, 5)}
    cs = sc.cases_of("targets")
    assert {c["fg_ratio"] for c in cs} == {0.0, 0.5, 1.0} and {c["hard_ratio"] for c in cs} == {0.0, 0.8, 1.0}
    assert {sc.aug_code(c) for c in cs} == {0, 1, 2, 3} and {type(c["aug"]) for c in cs} == {int, str}
    assert {c["state"] for c in cs} >= {(7, 0), (-1, 2 ** 40 + 3), None} and any(c["calls"] == 2 for c in cs)
    pcs = {(dict(f)["pc"] - c["m"] if dict(f)["pc"] >= c["m"] else min(dict(f)["pc"], 1)) for c in cs for f in c["frames"]}
    gcs = {(dict(f)["gc"] - c["g"] if dict(f)["gc"] >= c["g"] and c["g"] else min(dict(f)["gc"], 1)) for c in cs for f in c["frames"]}
    assert {-2, 0, 3} <= pcs and {-1, 0, 2} <= gcs
    assert any(dict(f)["twin_gt"] for c in cs for f in c["frames"]) and any(dict(f)["twin_roi"] for c in cs for f in c["frames"])


def test_first_argmax_wins_for_twin_rows():
    for c in sc.cases_of("targets"):
        t = sc.make_inputs(c)
        for f, fr in enumerate(dict(x) for x in c["frames"]):
            iou = t["mats"][f][0]
            if fr["twin_gt"] and iou.shape[1] >= 2:
                assert np.array_equal(iou[:, 0], iou[:, 1]) and (iou[:, 0] > 0).any()
                assert not (iou.argmax(1) == 1).any()
            if fr["twin_roi"] and iou.shape[0] >= 2:
                rows = t["proposals"][f, :iou.shape[0]]
                same = [(i, j) for i in range(len(rows)) for j in range(i + 1, len(rows)) if (rows[i] == rows[j]).all()]
                assert same and all(np.array_equal(iou[i], iou[j]) for i, j in same)


# ------------------------------------------------------------------------------------------------ the permutation
@pytest.mark.parametrize("n", list(range(1, 301)) + [4096, 4097, 16384, 65537, 2 ** 20])
def test_permutation_is_a_bijection(n):
    for k in range(3 if n <= 300 else 2):
        key = sc.rb_key(5, k, n % 7, sc.SHUFFLE)
        out = sc.rb_apply(key, n, np.arange(n))
        assert out.min() == 0 and out.max() == n - 1 and len(np.unique(out)) == n


def test_permutation_bit_count():
    assert [sc.perm_bits(n) for n in (1, 2, 4, 5, 16, 17, 64, 65, 256, 257, 1000, 1024, 1025, 16384)] == [2, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 10, 12, 14]


def test_mixer_known_values():
    """splitmix64's published first outputs for seed 0 (the state advances by the golden-ratio constant, which mix() adds itself)"""
    g = 0x9e3779b97f4a7c15
    assert [int(sc.mix(sc.u64(k * g))) for k in range(3)] == [0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]


# ------------------------------------------------------------------------------------------------ statistics of the streams
def test_near_point_inclusion_rate():
    """P < n with nf <= P: a near point is kept with probability (P - nf) / nn"""
    keys = call_keys(11, 4000, 2, sc.NEAR)
    for nn, m in ((100, 30), (1000, 744), (64, 1)):
        for rank in (0, nn // 2, nn - 1):
            q = sc.rb_apply(keys, nn, np.full(len(keys), rank))
            kept = int((q < m).sum())
            assert abs(kept - len(keys) * m / nn) <= binomial_band(len(keys), m / nn), (nn, m, rank, kept)


@pytest.mark.parametrize("n,count", [(64, 6400), (300, 30000)])
def test_shuffle_position_is_uniform(n, count):
    keys = call_keys(13, count, 1, sc.SHUFFLE)
    for x in (0, n // 3, n - 1):
        pos = sc.rb_apply(keys, n, np.full(count, x))
        assert chi2(np.bincount(pos, minlength=n), count / n) <= chi2_band(n - 1), (n, x)


def test_fisher_yates_prefix_is_a_uniform_subset():
    nfg, k, count = 6, 2, 6000
    seen = collections.Counter()
    for call in range(count):
        key, fg = sc.tgt_key(3, call), list(range(nfg))
        for s in range(k):
            j = s + int(sc.tgt_index(sc.tgt_uniform(key, 1, s, sc.DRAW_PERM), nfg - s))
            fg[s], fg[j] = fg[j], fg[s]
        seen[frozenset(fg[:k])] += 1
    assert len(seen) == 15
    assert chi2(list(seen.values()), count / 15) <= chi2_band(14)


def test_index_keep_and_row_draws():
    key, slots = sc.tgt_key(9, 4), np.arange(20000)
    idx = sc.tgt_index(sc.tgt_uniform(key, 3, slots, sc.DRAW_INDEX), 7)
    assert idx.min() == 0 and idx.max() == 6 and chi2(np.bincount(idx, minlength=7), len(slots) / 7) <= chi2_band(6)
    keep = int((sc.tgt_uniform(key, 3, slots, sc.DRAW_JITTER) < np.float32(0.2)).sum())
    assert abs(keep - 0.2 * len(slots)) <= binomial_band(len(slots), 0.2)
    row = sc.tgt_index(sc.tgt_uniform(key, 3, slots, sc.DRAW_JITTER + 16 + 1), 5)
    assert chi2(np.bincount(row, minlength=5), len(slots) / 5) <= chi2_band(4)
    far = sc.rb_index(sc.rb_key(9, 4, 0, sc.DRAW), slots, 11)
    assert far.min() == 0 and far.max() == 10 and chi2(np.bincount(far, minlength=11), len(slots) / 11) <= chi2_band(10)
    u = sc.tgt_uniform(key, 0, slots, 5)
    assert u.dtype == np.float32 and u.min() >= 0 and u.max() < 1
    assert sc.tgt_index(np.float32(1.0 - 2.0 ** -24), 3) == 2 and sc.tgt_index(np.float32(0.99999994), 16777216) == 16777215


def test_image_normals_are_standard():
    z = np.concatenate([sc.image_normals(sc.rb_key(21, k, k % 5, sc.NORMAL)) for k in range(4000)])
    n = len(z)
    assert abs(z.mean()) <= 6 / np.sqrt(n) and abs(z.var() - 1) <= 6 * np.sqrt(2 / n)
    assert np.isfinite(z).all()


def test_rng_state_is_read_as_uint64():
    assert sc.state_after([-1, 2 ** 40 + 3]).tolist() == [-1, 2 ** 40 + 4]
    assert sc.state_after([7, -1]).tolist() == [7, 0]
    assert sc.state_after([7, 2 ** 63 - 1]).tolist() == [7, -2 ** 63]
    assert int(sc.tgt_key(-1, 0)) == int(sc.tgt_key(2 ** 64 - 1, 0)) != int(sc.tgt_key(1, 0))


# ------------------------------------------------------------------------------------------------ the fp64 IoU
def test_ref_iou3d_hand_answers():
    a = np.array([1.0, 1.5, 10.0, 2.0, 1.0, 1.0, 0.3])
    assert abs(sc.ref_iou3d(a, a) - 1) < 1e-12
    b0 = np.array([0.0, 0.0, 0.0, 2.0, 1.0, 1.0, 0.0])
    assert abs(sc.ref_iou3d(b0, b0 + [1, 0, 0, 0, 0, 0, 0]) - 1 / 3) < 1e-12                # half shifted along l
    c0 = np.array([0.0, 0.0, 0.0, 4.0, 1.0, 1.0, 0.0])
    assert abs(sc.ref_iou3d(c0, c0 + [0, 0, 0, 0, 0, 0, np.pi / 2]) - 1 / 7) < 1e-12      # crossed at 90 degrees
    assert sc.ref_iou3d(b0, b0 + [0, 1.0, 0, 0, 0, 0, 0]) == 0                             # touching in height only
    assert sc.ref_iou3d(b0, b0 + [0, -3.0, 0, 0, 0, 0, 0]) == 0
    flat = b0.copy()
    flat[4] = 0.0
    assert sc.ref_iou3d(flat, b0) == 0 and sc.ref_iou3d(b0, flat) == 0                     # a zero-width box
    assert abs(sc.ref_iou3d(b0, b0 + [0, 0.5, 0, 0, 0, 0, 0]) - 1 / 3) < 1e-12            # half shifted in height


def test_ref_iou3d_is_symmetric_and_the_float32_form_stays_close(oracle_mod):
    worst = 0.0
    for c in sc.cases_of("targets"):
        t = sc.make_inputs(c)
        for f, (iou, gap, oh) in enumerate(t["mats"]):
            n, ng = iou.shape
            if not n or not ng:
                continue
            props, gts = t["proposals"][f, :n], t["gt"][f, :ng, :7]
            ij = np.argwhere(iou > 0)[:40]
            for i, j in ij:
                assert abs(sc.ref_iou3d(gts[j].astype(np.float64), props[i].astype(np.float64)) - iou[i, j]) < 1e-12
            assert (iou[(gap > 0) | (oh == 0)] == 0).all()
            worst = max(worst, float(np.abs(sc.f32_iou3d(oracle_mod, props, gts).astype(np.float64) - iou).max()))
    print("largest |float32 oracle composition - fp64 reference| over the table: %.3g" % worst)
    assert worst <= 1e-4


def test_gap_agrees_with_the_clip():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.uniform(-3, 3, (60, 1)), np.zeros((60, 1)), rng.uniform(-3, 3, (60, 1)), rng.uniform(0.5, 4, (60, 2)), np.ones((60, 1)),
                        rng.uniform(-np.pi, np.pi, (60, 1))], 1)
    gap = sc.bev_gap(a, a)
    for i in range(60):
        for j in range(60):
            assert (sc.ref_iou3d(a[i], a[j]) > 0) == (gap[i, j] < 0) or abs(gap[i, j]) < 1e-9


# ------------------------------------------------------------------------------------------------ limits and layout
def test_restated_limits_and_layout_equal_the_library():
    from heterofusionrcnn_amd import _lib, kitti_data as KD
    from heterofusionrcnn_amd import rcnn_train as RT
    L = _lib.lib()
    for b, m, g in ((1, 1, 1), (2, 5, 0), (3, 64, 3), (2, 257, 5), (1, 512, 128), (4, 40, 4), (1024, 512, 128)):
        assert L.hf_rcnn_targets_workspace(b, m, g) == sc.rcnn_targets_workspace(b, m, g)
    for b, total, mx in ((1, 1, 1), (5, 193, 65), (4, 2026, 1000), (5, 3514, 1000), (2, 0, 0), (3, 700, 257)):
        assert L.hf_rpn_batch_points_workspace(b, total, mx) == sc.rpn_points_workspace(b, total, mx)
    for b, px in ((1, 1), (4, 4096), (4, 4097), (5, 20), (2, 0), (3, 8192 * 1024)):
        assert L.hf_rpn_batch_image_workspace(b, px) == sc.rpn_image_workspace(b, px)
    for c in sc.cases_of("points"):
        t = sc.make_inputs(c)
        assert L.hf_rpn_batch_points_workspace(len(c["frames"]), t["total"], t["max_frame"]) == sc.rpn_points_workspace(len(c["frames"]), t["total"], t["max_frame"]) > 0
    assert (KD.STATUS_EMPTY, KD.STATUS_TOO_MANY_FAR) == (sc.STATUS_EMPTY, sc.STATUS_TOO_MANY_FAR)
    assert RT.AUG_METHODS == sc.AUG_METHODS
    assert float(np.float32(KD.EXPAND_GT_SIZE)) == float(np.float32(0.2))
    tc = RT.RcnnTrainConfig()
    c = sc.cases_of("targets")[0]
    assert (tc.cls_neg_iou_range, tc.cls_pos_iou_range[0], tc.reg_pos_iou_range[0]) == ((0.05, 0.45), c["pos"][0], c["pos"][1])
