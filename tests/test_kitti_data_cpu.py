"""CPU tests (-m "not gpu") of the RPN training batches (heterofusionrcnn_amd/kitti_data.py): the sample list against
kitti_dataset.py:113-129 (augmentation combinations, unlabelled frames dropped, per-epoch shuffle, rank shards), the host flips
against kitti_aug.py's formulas, the label rules of the NumPy restatement (tests/kitti_data_np.py) on hand-built boxes, and the
argument checks of the new C entry points (HF_EINVAL before any device work)."""
import os

import numpy as np
import pytest

from heterofusionrcnn_amd import _lib
from heterofusionrcnn_amd import kitti_data as KD

import kitti_data_np as KN

LABEL = "%s 0.00 0 -0.20 712.40 143.00 810.73 307.92 1.89 0.48 1.20 1.84 1.47 8.41 0.01\n"


def _dataset(tmp_path, labels):
    for name, types in labels.items():
        os.makedirs(tmp_path / "label_2", exist_ok=True)
        with open(tmp_path / "label_2" / (name + ".txt"), "w") as f:
            for t in types:
                f.write(LABEL % t)
    return str(tmp_path)


def test_aug_combinations_follow_the_reference_order():
    assert KD.aug_combinations(("flipping", "pca_jitter")) == [(), ("flipping",), ("pca_jitter",), ("flipping", "pca_jitter")]
    assert KD.aug_combinations(()) == [()]
    s = KD.build_sample_list(["a", "b"], ("flipping",))
    assert s == [("a", ()), ("b", ()), ("a", ("flipping",)), ("b", ("flipping",))]


def test_sample_list_drops_unlabelled_frames_and_reshuffles(tmp_path):
    root = _dataset(tmp_path, {"000000": ["Car"], "000001": ["DontCare"], "000002": ["Pedestrian", "Van"], "000003": []})
    sl = KD.SampleList(root, ["000000", "000001", "000002", "000003"], KD.CLASSES, seed=3)
    assert sl.dropped == ["000001", "000003"]
    assert len(sl) == 2 * 4
    assert sorted(set(n for n, _ in sl.samples)) == ["000000", "000002"]
    first = list(sl.order)
    assert sorted(first) == list(range(8))
    got = sl.take(8)
    assert got == [sl.samples[i] for i in first]
    sl.take(1)                      # crosses into epoch 2: a fresh permutation
    assert sl.epoch == 2 and sorted(sl.order) == list(range(8))
    orders = {tuple(first)}
    for _ in range(5):
        sl.next_epoch()
        orders.add(tuple(sl.order))
    assert len(orders) > 1
    again = KD.SampleList(root, ["000000", "000001", "000002", "000003"], KD.CLASSES, seed=3)
    assert again.order == first     # seeded


def test_rank_shards_are_disjoint_and_cover_the_list(tmp_path):
    names = ["%06d" % i for i in range(7)]
    root = _dataset(tmp_path, {n: ["Car"] for n in names})
    shards = [KD.SampleList(root, names, KD.CLASSES, seed=1, rank=r, world=3) for r in range(3)]
    ids = [i for s in shards for i in s.order]
    assert sorted(ids) == list(range(len(shards[0].samples)))
    full = KD.SampleList(root, names, KD.CLASSES, seed=1).order
    for r, s in enumerate(shards):
        assert s.order == full[r::3]


def test_split_file(tmp_path):
    root = _dataset(tmp_path, {"000000": ["Car"]})
    with open(tmp_path / "train.txt", "w") as f:
        f.write("000000\n\n")
    assert KD.read_split(root, "train") == ["000000"]
    assert KD.read_split(root, str(tmp_path / "train.txt")) == ["000000"]
    with pytest.raises(FileNotFoundError):
        KD.read_split(root, "val")


def test_host_flips_match_kitti_aug():
    rng = np.random.default_rng(0)
    boxes = rng.uniform(-3, 3, (20, 7))
    boxes[0, 6] = 0.0
    boxes[1, 6] = -0.0
    f = KD.flip_boxes_3d(boxes)
    for b, g in zip(boxes, f):
        ry = np.pi - b[6] if b[6] >= 0 else -np.pi - b[6]
        assert g[0] == -b[0] and g[1] == b[1] and g[2] == b[2] and g[6] == ry and np.array_equal(g[3:6], b[3:6])
    p2 = rng.uniform(-100, 700, (3, 4))
    fp = KD.flip_p2(p2, (375, 1242))
    assert fp[0, 2] == 1242 - p2[0, 2] and fp[0, 3] == -p2[0, 3]
    mask = np.ones((3, 4), bool)
    mask[0, 2:] = False
    assert np.array_equal(fp[mask], p2[mask])


def test_velo_to_rect_matrix_is_kitti_io_composition():
    rng = np.random.default_rng(1)
    calib = {"r0_rect": rng.standard_normal((3, 3)), "tr_velo_to_cam": rng.standard_normal((3, 4))}
    pts = rng.standard_normal((50, 3)) * 20
    from heterofusionrcnn_amd import kitti_io
    m = KD.velo_to_rect_matrix(calib)
    np.testing.assert_allclose(pts @ m[:, :3].T + m[:, 3], kitti_io.lidar_to_rect(pts, calib), rtol=0, atol=1e-9)


# ------------------------------------------------------------------ label rules (the restatement the GPU test holds the kernel to)
def hand_boxes():
    """two overlapping boxes of classes 1 and 2, axis-aligned (ry 0): box 1 spans x in (-1, 1), y in (-1, 0), z in (-2, 2);
    box 2 is box 1 shifted by +0.3 in x"""
    return np.array([[0.0, 0.0, 0.0, 2.0, 4.0, 1.0, 0.0], [0.3, 0.0, 0.0, 2.0, 4.0, 1.0, 0.0]]), np.array([1, 2], np.int32)


def test_label_rules_last_box_wins():
    boxes, cls = hand_boxes()
    pts = np.array([[0.5, -0.5, 0.0],      # inside both: the later box
                    [-0.8, -0.5, 0.0],     # inside box 1, 0.1 outside box 2 (x > -0.7): box 2's ring overrides
                    [-0.95, -0.5, 0.0],    # inside box 1, outside box 2 and its enlarged box (x > -0.9): box 1's class
                    [5.0, -0.5, 0.0]])     # outside everything
    c, r, _ = KN.rpn_labels(pts, boxes, cls)
    assert c.tolist() == [2, -1, 1, 0]
    np.testing.assert_array_equal(r[0], boxes[1].astype(np.float32))
    np.testing.assert_array_equal(r[1], boxes[0].astype(np.float32))   # the ring keeps the box it was labelled with
    np.testing.assert_array_equal(r[3], np.zeros(7, np.float32))


def test_label_rules_ring_overrides_earlier_foreground():
    boxes, cls = hand_boxes()
    pts = np.array([[-0.8, -0.5, 0.0]])    # inside box 1, 0.1 outside box 2's x face -> box 2's ring
    c, _, _ = KN.rpn_labels(pts, boxes, cls)
    assert c.tolist() == [-1]
    c1, _, _ = KN.rpn_labels(pts, boxes[:1], cls[:1])
    assert c1.tolist() == [1]


def test_label_rules_strict_faces():
    box = np.array([[0.0, 0.0, 0.0, 2.0, 4.0, 1.0, 0.0]])
    pts = np.array([[1.0, -0.5, 0.0],      # on the x face: not inside, inside the enlarged box -> ring
                    [0.0, 0.0, 0.0],       # on the bottom face (y = 0): ring
                    [0.0, -0.2, 1.9],      # inside
                    [0.0, 0.2, 0.0],       # on the enlarged box's bottom face (y + expand): outside
                    [1.25, -0.5, 0.0]])    # beyond the enlarged box's x face: outside
    c, _, _ = KN.rpn_labels(pts, box, np.array([3]))
    assert c.tolist() == [-1, -1, 3, 0, 0]


# ------------------------------------------------------------------ C entry points: argument checks without a GPU
def test_entry_points_reject_bad_arguments():
    L = _lib.lib()
    nul = None
    assert L.hf_rpn_batch_points_workspace(-1, 10, 10) == 0
    assert L.hf_rpn_batch_points_workspace(2, 10, 11) == 0          # a frame longer than the buffer
    assert L.hf_rpn_batch_points_workspace(2, 100, 50) > 0
    args = [nul] * 12
    assert L.hf_rpn_batch_points(2, 0, 100, 50, *args, 0, nul) == _lib.HF_EINVAL        # P = 0
    assert L.hf_rpn_batch_points(2, 16, 100, 200, *args, 0, nul) == _lib.HF_EINVAL      # max_frame_points > total
    assert L.hf_rpn_batch_points(2, 16, 100, 50, *args, 0, nul) == _lib.HF_EINVAL       # NULL pointers
    assert L.hf_rpn_batch_points(0, 16, 0, 0, *args, 0, nul) == _lib.HF_OK              # nothing to do
    assert L.hf_rpn_point_labels(2, 16, 129, *([nul] * 4), 0.2, nul, nul, nul) == _lib.HF_EINVAL   # g > 128
    assert L.hf_rpn_point_labels(2, 16, 4, *([nul] * 4), -1.0, nul, nul, nul) == _lib.HF_EINVAL    # negative expand
    assert L.hf_rpn_point_labels(2, 16, 4, *([nul] * 4), 0.2, nul, nul, nul) == _lib.HF_EINVAL     # NULL pointers
    assert L.hf_rpn_batch_image_workspace(2, 1 << 24) == 0
    assert L.hf_rpn_batch_image_workspace(2, 1242 * 375) > 0
    img = [nul] * 5
    assert L.hf_rpn_batch_image(2, 1242 * 375, 100, *img, 0, 1200, *img, 0, nul) == _lib.HF_EINVAL  # out_h = 0
    assert L.hf_rpn_batch_image(2, 1 << 24, 100, *img, 360, 1200, *img, 0, nul) == _lib.HF_EINVAL   # too many pixels
    assert L.hf_rpn_batch_image(2, 1000, 100, *img, 360, 1200, *img, 0, nul) == _lib.HF_EINVAL      # NULL pointers
