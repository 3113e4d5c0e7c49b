"""GPU tests of the RPN -> RCNN hand-off (csrc/rcnn_batch.hip, hf_box3d_iou_matrix, export_rpn, rcnn_data, train_rcnn) on the
four committed KITTI frames of tests/golden/kitti (scans decompressed into a temporary directory, synthetic PNGs written next
to them), held against the NumPy restatement in tests/rcnn_handoff_np.py and tests/kitti_data_np.py."""
import lzma
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from heterofusionrcnn_amd import kitti_data as KD
from heterofusionrcnn_amd import kitti_io, modules
from heterofusionrcnn_amd import rcnn_data as RD
from heterofusionrcnn_amd import rcnn_train as RT
from heterofusionrcnn_amd.inference import rescale_p2

import kitti_data_np as KN
import rcnn_handoff_np as HN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti")
NAMES = ["000000", "000001", "000002", "000003"]
SIZES = {"000000": (1242, 375), "000001": (1224, 370), "000002": (1242, 375), "000003": (1224, 370)}
HW = (360, 1200)
IMG_CONV = ((1, 16), (1, 16), (1, 16), (1, 16))


def _png(path, w, h, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 200.0 / w, yy * 200.0 / h, (xx + yy) * 100.0 / (w + h)], -1)
    img = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(path)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("kitti")
    for d in ("calib", "label_2"):
        shutil.copytree(os.path.join(GOLD, d), os.path.join(root, d))
    os.makedirs(os.path.join(root, "velodyne"))
    os.makedirs(os.path.join(root, "image_2"))
    for i, n in enumerate(NAMES):
        with lzma.open(os.path.join(GOLD, "velodyne", n + ".bin.xz")) as f, open(os.path.join(root, "velodyne", n + ".bin"), "wb") as g:
            g.write(f.read())
        _png(os.path.join(root, "image_2", n + ".png"), *SIZES[n], seed=i)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(NAMES) + "\n")
    return str(root)


@pytest.fixture(scope="module")
def handoff(dataset, tmp_path_factory):
    """a briefly trained RPN exported at batch 3 (the last batch is short) -> (out_dir, totals, {name: the device IoU the
    writer received})"""
    from heterofusionrcnn_amd import export_rpn, train_rpn
    out = str(tmp_path_factory.mktemp("handoff"))
    model_path = os.path.join(out, "rpn.pt")
    train_rpn.train(dataset, "train", steps=3, batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV, save=model_path)
    lines, seen = [], {}
    orig = export_rpn._write_batch

    def spy(out_dir, names, has_label, host, event, gcounts, bi, log):
        r = orig(out_dir, names, has_label, host, event, gcounts, bi, log)
        for i, n in enumerate(names):
            seen[n] = (host["iou"][i, :, :gcounts[i]].numpy().copy(), host["proposals"][i].numpy().copy())
        return r

    export_rpn._write_batch = spy
    try:
        totals = export_rpn.export(dataset, model_path, out, "train", batch=3, img_conv=IMG_CONV, workers=2, log=lines.append)
    finally:
        export_rpn._write_batch = orig
    assert len(lines) == 2 and all("Recall@3DIoU=0.5" in l for l in lines), lines
    return out, totals, seen


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("b,p,c", [(2, 16384, 288), (3, 1003, 21)])
def test_pack_split_round_trip_is_bit_exact(b, p, c):
    rng = np.random.default_rng(p + c)
    xyz = rng.standard_normal((b, p, 3)).astype(np.float32)
    inten = rng.standard_normal((b, p, 1)).astype(np.float32)
    fg = rng.random((b, p)) < 0.3
    fts = rng.standard_normal((b, p, c)).astype(np.float32)
    cu = lambda a: torch.from_numpy(a).cuda()
    rows = RD.handoff_pack(cu(xyz), cu(inten), cu(fg), cu(fts))
    exp = HN.pack(xyz, inten, fg, fts)
    assert np.array_equal(rows.cpu().numpy(), exp)
    for flip in ([0] * b, [1] * b, [f % 2 for f in range(b)]):
        got = RD.batch_inputs(rows, torch.tensor(flip, dtype=torch.int32, device="cuda"))
        want = HN.split(exp, flip)
        for g_, w_ in zip(got, want):
            assert np.array_equal(g_.cpu().numpy(), w_), flip
    # a fg value other than 0 / 1 sets the frame's status bit (read as fg = value != 0)
    bad = exp.copy()
    bad[b - 1, p // 2, 4] = 0.5
    got = RD.batch_inputs(cu(bad), torch.zeros(b, dtype=torch.int32, device="cuda"))
    assert got[4].cpu().tolist() == [0] * (b - 1) + [RD.STATUS_BAD_FG]
    assert bool(got[2][b - 1, p // 2])


def test_iou_matrix_equals_the_target_layer_and_box3d_iou(dataset):
    rng = np.random.default_rng(3)
    b, m, g = 4, 100, 12
    gt, gc = [], []
    for n in NAMES:
        boxes, cls = KD.read_frame_labels(dataset, n, list(KD.CLASSES))
        gt.append(boxes)
        gc.append(cls)
    gt_pad, gt_count = HN.pad_gt(gt, gc, g)
    props, counts = [], []
    for f in range(b):
        src = gt[f][rng.integers(0, len(gt[f]), m)]
        jit = src + rng.normal(0, 1, (m, 7)) * np.array([0.5, 0.1, 0.5, 0.3, 0.2, 0.2, 0.3])
        k = [m, 57, 1, m][f]
        props.append(jit[:k].astype(np.float32))
        counts.append(k)
    prop_pad, pc = HN.pad_proposals(props, m)
    cu = lambda a: torch.from_numpy(a).cuda()
    iou = RD.box3d_iou_matrix(cu(prop_pad), cu(pc), cu(gt_pad), cu(gt_count))
    _, iou_rois, _, _ = RT.proposal_targets(cu(prop_pad), cu(pc), cu(gt_pad), cu(gt_count), train=False)
    assert torch.equal(iou.max(dim=2).values, iou_rois), "the matrix's max is not the target layer's IoU"
    assert (iou > 0.3).sum() > 50
    for f in range(b):
        n, ng = counts[f], int(gt_count[f])
        ref = modules.box3d_iou(cu(props[f]), cu(gt_pad[f, :ng, :7].copy()))[0]
        assert torch.allclose(iou[f, :n, :ng], ref, rtol=0, atol=1e-5)
        assert (iou[f, n:] == 0).all() and (iou[f, :, ng:] == 0).all()


# ------------------------------------------------------------------------------------------------ export
def test_export_writes_the_three_files(dataset, handoff):
    out, totals, _ = handoff
    assert sorted(totals) == NAMES
    c = None
    for n in NAMES:
        paths = RD.handoff_paths(out, n)
        b, s = kitti_io.load_proposals_and_scores(paths["proposals"])
        assert b.shape == (100, 7) and s.shape == (100,)
        a = np.load(paths["features"])
        assert a.dtype == np.float32 and a.shape[0] == 16384 and a.shape[1] > 6
        c = a.shape[1] - 5 if c is None else c
        assert a.shape[1] == 5 + c
        assert set(np.unique(a[:, 4]).tolist()) <= {0.0, 1.0}
        boxes, cls = KD.read_frame_labels(dataset, n, list(KD.CLASSES))
        iou = np.loadtxt(paths["iou"]).reshape(-1, len(cls))
        assert iou.shape == (100, len(cls))
        assert totals[n]["labels"] == len(cls) and totals[n]["proposals"] == 100


def test_export_iou_file_matches_the_unrounded_device_iou(dataset, handoff):
    """the IoU the export computed on the device (captured from its writer) against the file: within the %.3f rounding"""
    out, _, seen = handoff
    assert sorted(seen) == NAMES
    for n in NAMES:
        iou, props = seen[n]
        boxes, cls = KD.read_frame_labels(dataset, n, list(KD.CLASSES))
        gt, gc = HN.pad_gt([boxes], [cls], len(cls))
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dev = RD.box3d_iou_matrix(cu(props[None]), cu(np.array([len(props)], np.int32)), cu(gt), cu(gc))[0].cpu().numpy()
        assert np.array_equal(dev, iou), "the written IoU is not the IoU of the unrounded proposals"
        f = np.loadtxt(RD.handoff_paths(out, n)["iou"]).reshape(-1, len(cls))
        assert f.shape == iou.shape and np.abs(f - iou).max() <= 5e-4 + 1e-6


# ------------------------------------------------------------------------------------------------ loader
def _expected(dataset, out, name, augs):
    rows = np.load(RD.handoff_paths(out, name)["features"])
    flip = "flipping" in augs
    props, _ = kitti_io.load_proposals_and_scores(RD.handoff_paths(out, name)["proposals"])
    boxes, cls = KD.read_frame_labels(dataset, name, list(KD.CLASSES))
    if flip:
        props, boxes = HN.flip_boxes(props), HN.flip_boxes(boxes)
    calib = kitti_io.read_calib(os.path.join(dataset, "calib", name + ".txt"))
    img = KD.read_png(os.path.join(dataset, "image_2", name + ".png"))
    h0, w0 = img.shape[:2]
    p2 = KD.flip_p2(calib["p2"], (h0, w0)) if flip else calib["p2"]
    return rows, flip, props.astype(np.float32), boxes.astype(np.float32), cls, rescale_p2(p2.astype(np.float32), (w0, h0), (HW[1], HW[0])), img


def _check_batch(bt, dataset, out, with_image=True):
    b = len(bt.names)
    m, g = bt.proposals.shape[1], bt.gt.shape[1]
    for f, (name, augs) in enumerate(zip(bt.names, bt.augs)):
        rows, flip, props, boxes, cls, calib, img = _expected(dataset, out, name, augs)
        want = HN.split(rows[None], [int(flip)])
        for got, w_ in zip((bt.xyz, bt.intensity, bt.fg_mask, bt.rpn_fts, bt.status), want):
            assert np.array_equal(got[f].cpu().numpy(), w_[0]), (name, augs)
        pp, pc = HN.pad_proposals([props], m)
        gg, gc = HN.pad_gt([boxes], [cls], g)
        assert np.array_equal(bt.proposals[f].cpu().numpy(), pp[0]) and int(bt.proposal_count[f]) == pc[0]
        assert np.array_equal(bt.gt[f].cpu().numpy(), gg[0]) and int(bt.gt_count[f]) == gc[0]
        assert np.array_equal(bt.calib[f].cpu().numpy(), calib)
        if with_image:
            assert np.array_equal(bt.image[f].cpu().numpy(), KN.image_sample(img, flip, None, HW)), name
    assert b == bt.xyz.shape[0]


def test_loader_train_mode_with_flipping(dataset, handoff):
    out, _, _ = handoff
    data = RD.KittiRcnnBatches(dataset, out, "train", mode="train", batch=4, seed=2, aug_list=("flipping",), workers=2)
    try:
        seen = []
        for _ in range(2):                     # one epoch: 4 frames x {(), (flipping,)}
            bt = data.next()
            _check_batch(bt, dataset, out)
            seen += list(zip(bt.names, bt.augs))
        assert sorted(seen) == sorted((n, a) for n in NAMES for a in [(), ("flipping",)])
        assert data.check_status() == {"bad_fg": 0}
    finally:
        data.close()


def test_loader_val_mode(dataset, handoff):
    out, _, _ = handoff
    data = RD.KittiRcnnBatches(dataset, out, "train", mode="val", batch=3, workers=2)
    try:
        batches = list(data)
    finally:
        data.close()
    assert [len(b.names) for b in batches] == [3, 1] and sum((b.names for b in batches), []) == NAMES
    for bt in batches:
        assert all(a == () for a in bt.augs)
        _check_batch(bt, dataset, out)
        for f, n in enumerate(bt.names):
            props, _ = kitti_io.load_proposals_and_scores(RD.handoff_paths(out, n)["proposals"])
            assert np.array_equal(bt.proposals[f].cpu().numpy(), props.astype(np.float32))


def test_loader_rejects_missing_and_mismatched_files(dataset, handoff, tmp_path):
    out, _, _ = handoff
    bad = str(tmp_path / "h")
    shutil.copytree(out, bad)
    os.remove(RD.handoff_paths(bad, "000002")["features"])
    with pytest.raises(FileNotFoundError, match="000002"):
        data = RD.KittiRcnnBatches(dataset, bad, NAMES, mode="val", batch=4, workers=2)
        try:
            data.next()
        finally:
            data.close()
    a = np.load(RD.handoff_paths(out, "000002")["features"])
    np.save(RD.handoff_paths(bad, "000002")["features"], a[:, :-1].copy())
    with pytest.raises(ValueError, match="000002"):
        data = RD.KittiRcnnBatches(dataset, bad, NAMES, mode="val", batch=4, workers=2)
        try:
            data.next()
        finally:
            data.close()


# ------------------------------------------------------------------------------------------------ training and the loop
def test_file_fed_captured_rcnn_training(dataset, handoff):
    from heterofusionrcnn_amd import train_rcnn
    out, _, _ = handoff
    logs = []
    losses, trainer = train_rcnn.train(dataset, out, "train", steps=30, batch=2, seed=1, log_every=10, workers=2, img_conv=IMG_CONV,
                                       log=logs.append)
    assert len(losses) == 30 and np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    assert len(logs) == 3 and " fg " in logs[0] and " bg " in logs[0]
    assert isinstance(trainer.model, RT.RcnnWithImageBranch)


def test_cli_export_then_train(dataset, tmp_path):
    from heterofusionrcnn_amd import train_rpn
    rpn_path, out, rcnn_path = str(tmp_path / "rpn.pt"), str(tmp_path / "handoff"), str(tmp_path / "rcnn.pt")
    train_rpn.train(dataset, "train", steps=1, batch=2, config="rpn_multiclass_points", log_every=0, workers=2, save=rpn_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "heterofusionrcnn_amd.export_rpn", dataset, rpn_path, out,
                        "--config", "rpn_multiclass_points", "--batch", "3", "--workers", "2"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "done: 4 frames" in r.stdout and "Recall@3DIoU=0.5" in r.stdout
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "heterofusionrcnn_amd.train_rcnn", dataset, out, "--steps",
                        "3", "--log-every", "1", "--workers", "2", "--save", rcnn_path], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "done: 3 steps" in r.stdout
    sd = torch.load(rcnn_path, map_location="cpu")
    assert any(k.startswith("model.img_net.") for k in sd) and any(k.startswith("model.rcnn.") for k in sd) and "rng_state" in sd


def test_second_stage_from_the_handoff_writes_results(dataset, handoff, tmp_path):
    from heterofusionrcnn_amd import kitti_eval, train_rcnn
    out, _, _ = handoff
    c = RD.feature_shape(RD.handoff_paths(out, NAMES[0])["features"])[1] - 5
    trainer = train_rcnn.make_trainer(c, IMG_CONV, seed=0)
    res_dir = str(tmp_path / "results")
    written = RD.run_rcnn_from_handoff(trainer, dataset, out, NAMES, res_dir, batch=3, workers=2)
    assert sorted(written) == NAMES and trainer.training
    for n in NAMES:
        with open(os.path.join(res_dir, n + ".txt")) as f:
            lines = [l.split() for l in f if l.strip()]
        assert len(lines) == written[n] and all(len(l) == 16 for l in lines)
    res = kitti_eval.evaluate_dirs(os.path.join(dataset, "label_2"), res_dir)
    assert res["ap"].shape == (3, 3, 3) and len(res["frames"]) == 4


def test_export_and_second_stage_leave_no_worker_thread(dataset, handoff, tmp_path):
    """the reader threads (hf-read...) and the write-back threads (hf-write...) end with the call that started them"""
    from heterofusionrcnn_amd import export_rpn, train_rcnn
    workers = lambda: [t.name for t in threading.enumerate() if t.name.startswith(("hf-read", "hf-write"))]
    out, _, _ = handoff
    c = RD.feature_shape(RD.handoff_paths(out, NAMES[0])["features"])[1] - 5
    written = RD.run_rcnn_from_handoff(train_rcnn.make_trainer(c, IMG_CONV, seed=0), dataset, out, NAMES, str(tmp_path / "results"),
                                       batch=2, workers=2)
    assert sorted(written) == NAMES and workers() == []
    totals = export_rpn.export(dataset, os.path.join(out, "rpn.pt"), str(tmp_path / "handoff"), "train", batch=2, img_conv=IMG_CONV,
                               workers=2, log=None)
    assert sorted(totals) == NAMES and workers() == []


def test_a_failed_capture_leaves_no_loader_thread(dataset, handoff, monkeypatch):
    """train_rcnn.train whose step cannot be built (the loop's TrainStep raises) closes the loader it opened: none of its reader
    (hf-read-pool...) or read-ahead (hf-read-ahead...) threads survives the call, and the caller gets the exception as raised"""
    from heterofusionrcnn_amd import train_loop, train_rcnn
    readers = lambda: [t.name for t in threading.enumerate() if t.name.startswith("hf-read")]
    refused = RuntimeError("the step cannot be captured")

    def no_step(*args, **kwargs):
        raise refused

    monkeypatch.setattr(train_loop, "TrainStep", no_step)
    assert readers() == []
    with pytest.raises(RuntimeError) as caught:
        train_rcnn.train(dataset, handoff[0], "train", steps=2, batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV)
    assert caught.value is refused and readers() == []
