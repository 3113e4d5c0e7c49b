"""CPU tests (-m "not gpu") of the RPN -> RCNN hand-off: argument checks of the new C entry points (HF_EINVAL before any HIP
call), the .npy header parse + readinto of rcnn_data against np.load, the RCNN sample list (unlabelled frames dropped, the
reference's augmentation combinations), and the formats the export writes (kitti_dataset.py:238-252, :467)."""
import os

import numpy as np
import pytest

from heterofusionrcnn_amd import _lib, export_rpn, kitti_io
from heterofusionrcnn_amd import kitti_data as KD
from heterofusionrcnn_amd import rcnn_data as RD

import rcnn_handoff_np as HN

LABEL = "%s 0.00 0 -0.20 712.40 143.00 810.73 307.92 1.89 0.48 1.20 1.84 1.47 8.41 0.01\n"


def test_entry_points_refuse_out_of_limit_arguments():
    L = _lib.lib()
    E = _lib.HF_EINVAL
    for b, p, c in ((1025, 4, 4), (-1, 4, 4), (1, 0, 4), (1, (1 << 20) + 1, 4), (1, 4, 0), (1, 4, 4097)):
        assert L.hf_rpn_handoff_pack(b, p, c, None, None, None, None, None, None) == E, (b, p, c)
        assert L.hf_rcnn_batch_inputs(b, p, c, None, None, None, None, None, None, None, None) == E, (b, p, c)
    # in range but null pointers: refused too, still before any device work
    assert L.hf_rpn_handoff_pack(2, 16, 8, None, None, None, None, None, None) == E
    assert L.hf_rcnn_batch_inputs(2, 16, 8, None, None, None, None, None, None, None, None) == E
    for b, m, g in ((1025, 4, 4), (1, 0, 4), (1, 513, 4), (1, 4, 129), (1, 4, -1)):
        assert L.hf_box3d_iou_matrix(b, m, g, None, None, None, None, None, None) == E, (b, m, g)
    assert L.hf_box3d_iou_matrix(2, 100, 4, None, None, None, None, None, None) == E
    assert L.hf_box3d_iou_matrix(0, 100, 4, None, None, None, None, None, None) == _lib.HF_OK


@pytest.mark.parametrize("p,c", [(1003, 21), (64, 288)])
def test_header_parse_and_readinto_equal_np_load(tmp_path, p, c):
    rng = np.random.default_rng(p)
    arr = rng.standard_normal((p, 5 + c)).astype(np.float32)
    path = str(tmp_path / "x.npy")
    np.save(path, arr)
    assert RD.feature_shape(path) == (p, 5 + c)
    out = np.full((p, 5 + c), np.nan, np.float32)
    RD.read_npy_into(path, out, (p, 5 + c), "x")
    assert np.array_equal(out, np.load(path))
    with pytest.raises(ValueError, match="frame y"):
        RD.read_npy_into(path, out[:-1], (p - 1, 5 + c), "y")
    with pytest.raises(FileNotFoundError, match="frame z"):
        RD.read_npy_into(str(tmp_path / "missing.npy"), out, (p, 5 + c), "z")
    np.save(path, arr.astype(np.float64))
    with pytest.raises(ValueError):
        RD.feature_shape(path)


def test_sample_list_drops_unlabelled_frames_and_keeps_the_aug_combinations(tmp_path):
    os.makedirs(tmp_path / "label_2")
    for name, types in {"000000": ["Car"], "000001": ["DontCare"], "000002": ["Cyclist", "Van"], "000003": []}.items():
        with open(tmp_path / "label_2" / (name + ".txt"), "w") as f:
            f.writelines(LABEL % t for t in types)
    sl = KD.SampleList(str(tmp_path), ["000000", "000001", "000002", "000003"], KD.CLASSES, aug_list=("flipping", "pca_jitter"))
    assert sl.dropped == ["000001", "000003"]
    assert sl.samples == [(n, a) for a in [(), ("flipping",), ("pca_jitter",), ("flipping", "pca_jitter")] for n in ("000000", "000002")]


def test_export_writers_produce_the_reference_formats(tmp_path):
    rng = np.random.default_rng(1)
    n, g, p, c = 100, 3, 257, 13
    props = rng.uniform(-5, 5, (n, 7)).astype(np.float32)
    scores = rng.uniform(0, 1, n).astype(np.float32)
    iou = rng.uniform(0, 1, (1, n, g)).astype(np.float32)
    xyz, inten = rng.standard_normal((1, p, 3)).astype(np.float32), rng.standard_normal((1, p, 1)).astype(np.float32)
    fg, fts = rng.random((1, p)) < 0.3, rng.standard_normal((1, p, c)).astype(np.float32)
    rows = HN.pack(xyz, inten, fg, fts)
    import torch
    host = {"rows": torch.from_numpy(rows), "proposals": torch.from_numpy(props[None]), "scores": torch.from_numpy(scores[None]),
            "iou": torch.from_numpy(iou)}

    class _Done:
        def synchronize(self):
            pass

    for d in RD.HANDOFF_DIRS:
        os.makedirs(tmp_path / d)
    tot = export_rpn._write_batch(str(tmp_path), ["000007"], [True], host, _Done(), [g], 0, None)
    txt = open(tmp_path / "proposals_and_scores" / "000007.txt").read().split("\n")
    assert len([l for l in txt if l]) == n and all(len(l.split()) == 8 for l in txt if l)
    assert all(len(v.split(".")[1]) == 3 for v in txt[0].split())
    b, s = kitti_io.load_proposals_and_scores(str(tmp_path / "proposals_and_scores" / "000007.txt"))
    assert np.abs(b - props).max() <= 5e-4 + 1e-6 and np.abs(s - scores).max() <= 5e-4 + 1e-6
    a = np.load(str(tmp_path / "rpn_feature" / "000007.npy"))
    assert a.dtype == np.float32 and a.shape == (p, 5 + c) and np.array_equal(a, rows[0])
    f = kitti_io.load_rpn_features(str(tmp_path / "rpn_feature" / "000007.npy"), c)
    assert np.array_equal(f["pts_fts"], fts[0]) and np.array_equal(f["fg_mask"], fg[0].astype(np.float32))
    m = np.loadtxt(str(tmp_path / "proposals_iou" / "000007.txt")).reshape(-1, g)      # kitti_dataset.py:467
    assert m.shape == (n, g) and np.abs(m - iou[0]).max() <= 5e-4 + 1e-6
    best = iou[0].max(axis=0)
    assert tot["000007"] == {"proposals": n, "labels": g, "recall_50": int((best > 0.5).sum()), "recall_70": int((best > 0.7).sum())}


def test_restatement_round_trip_and_flip():
    rng = np.random.default_rng(2)
    xyz, inten = rng.standard_normal((2, 9, 3)).astype(np.float32), rng.standard_normal((2, 9, 1)).astype(np.float32)
    fg, fts = rng.random((2, 9)) < 0.5, rng.standard_normal((2, 9, 5)).astype(np.float32)
    x, i, m, f, st = HN.split(HN.pack(xyz, inten, fg, fts), [0, 1])
    assert np.array_equal(x[0], xyz[0]) and np.array_equal(x[1, :, 0], -xyz[1, :, 0]) and np.array_equal(i, inten)
    assert np.array_equal(m, fg) and np.array_equal(f, fts) and st.tolist() == [0, 0]
