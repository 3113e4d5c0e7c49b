"""GPU tests of heterofusionrcnn_amd/validate.py on the four committed KITTI frames (tests/validate_fixtures.py): validate_rpn against
export_rpn.export's totals and against the loss and accuracy the test evaluates itself in eval mode on batches drawn the same way,
validate_rcnn likewise against proposal_targets(train=False) + rcnn_loss_fused, and the command line over a checkpoint directory."""
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import validate_fixtures as VF  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = VF.ROOT
NAMES = VF.NAMES


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    return VF.build_dataset(tmp_path_factory.mktemp("kitti"))


@pytest.fixture(scope="module")
def handoff(dataset, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("handoff"))
    model_path, totals = VF.build_handoff(dataset, out)
    return out, model_path, totals


@pytest.fixture(scope="module")
def rpn_result(dataset, handoff):
    from heterofusionrcnn_amd import validate
    _, model_path, _ = handoff
    return validate.validate_rpn(dataset, model_path, "train", batch=VF.EXPORT_BATCH, seed=VF.SEED, workers=2, img_conv=VF.IMG_CONV)


def test_validate_rpn_counts_equal_the_export(handoff, rpn_result):
    _, _, totals = handoff
    assert rpn_result["names"] == NAMES and rpn_result["batch_frames"] == [3, 1]
    for n in NAMES:
        got = rpn_result["frames"][n]
        assert {k: got[k] for k in ("proposals", "labels", "recall_50", "recall_70")} == totals[n], n
        assert got["points"] == 16384 and 0 <= got["correct"] <= 16384
        assert got["sum_iou3d"] >= 0.0 and got["sum_iou2d"] >= 0.0 and np.isfinite(got["sum_angle"])
    tot = rpn_result["totals"]
    labels = sum(t["labels"] for t in totals.values())
    assert tot["frames"] == 4 and tot["labels"] == labels and tot["avg_proposals"] == 100.0
    assert tot["recall_50"] == sum(t["recall_50"] for t in totals.values()) / labels
    assert tot["recall_70"] == sum(t["recall_70"] for t in totals.values()) / labels


def test_validate_rpn_losses_and_accuracy(dataset, handoff, rpn_result):
    """the per-batch losses are rpn_loss_parts in eval mode on the same batches, the averages their frame-weighted mean, the
    correct points torch's argmax against max(label, 0)"""
    from heterofusionrcnn_amd import export_rpn, validate
    from heterofusionrcnn_amd import kitti_data as KD
    from heterofusionrcnn_amd.graph_step import rpn_loss_parts
    _, model_path, _ = handoff
    net = export_rpn.load_rpn(model_path, "rpn_multiclass", VF.IMG_CONV).eval()
    batches = export_rpn.proposals_from_files(net, dataset, NAMES, VF.EXPORT_BATCH, 2, VF.SEED, 16384, VF.HW, (9000, 0.8, 100), KD.CLASSES)
    losses, correct, frames = [], [], []
    try:
        with torch.no_grad():
            for _, meta, xyz, inten, image, _ in batches:
                label_cls, label_reg = KD.point_labels(xyz, meta["boxes"], meta["cls"], meta["gt_count"])
                inputs = {"xyz": xyz, "intensity": inten, "label_cls": label_cls, "label_reg": label_reg, "img_fts": image,
                          "calib": meta["calib"]}
                loss, parts = rpn_loss_parts(net, inputs, net.geometry(xyz))
                losses.append([float(parts["segmentation"]), float(parts["bin_classification"]), float(parts["regression"]), float(loss)])
                seg, _ = net(xyz, inten, geometry=net.geometry(xyz), img_fts=image, calib=meta["calib"])
                correct += (seg.argmax(dim=-1) == label_cls.clamp(min=0)).sum(dim=1).tolist()
                frames.append(xyz.shape[0])
    finally:
        batches.close()
    want = np.asarray(losses, np.float32)
    got = rpn_result["batch_losses"]
    print("\nper-batch losses %s\nthe test's %s\nlargest difference %g" % (got.tolist(), want.tolist(), np.abs(got - want).max()))
    assert np.isfinite(got).all() and (got > 0).all()
    assert np.array_equal(got, want), "the validation losses are not rpn_loss_parts of the same batches, bit for bit"
    avg = (want.astype(np.float64) * np.asarray(frames, np.float64)[:, None]).sum(axis=0) / sum(frames)
    for k, v in zip(validate.RPN_LOSSES, avg):
        assert rpn_result["totals"][k] == float(v), k
    assert rpn_result["rows"]["correct"].tolist() == correct
    assert rpn_result["totals"]["seg_accuracy"] == sum(correct) / (4 * 16384)
    assert net.training is False


def test_validate_rpn_restores_the_training_mode(dataset, handoff):
    from heterofusionrcnn_amd import export_rpn, validate
    net = export_rpn.load_rpn(handoff[1], "rpn_multiclass", VF.IMG_CONV).train()
    res = validate.validate_rpn(dataset, net, ["000001"], batch=2, workers=2, img_conv=VF.IMG_CONV)
    assert net.training and res["names"] == ["000001"] and res["batch_frames"] == [1]


def test_validate_rcnn_against_the_target_layer_and_the_fused_loss(dataset, handoff, tmp_path):
    from heterofusionrcnn_amd import rcnn_data as RD
    from heterofusionrcnn_amd import rcnn_train as RT
    from heterofusionrcnn_amd import kitti_data as KD
    from heterofusionrcnn_amd import kitti_io, train_rcnn, validate
    # the hand-off of a three-step RPN holds no proposal near a label: a copy whose first rows are jittered labels, so that the
    # regression masks are not empty
    out = str(tmp_path / "handoff")
    shutil.copytree(handoff[0], out)
    rng = np.random.default_rng(11)
    for n in NAMES:
        path = RD.handoff_paths(out, n)["proposals"]
        props, scores = kitti_io.load_proposals_and_scores(path)
        boxes, _ = KD.read_frame_labels(dataset, n, list(KD.CLASSES))
        k = len(boxes)
        props[:k] = boxes + rng.normal(0, 0.05, (k, 7))
        props[k:2 * k] = boxes + rng.normal(0, 0.3, (k, 7))
        kitti_io.save_proposals_and_scores(path, props, scores)
    c = RD.feature_shape(RD.handoff_paths(out, NAMES[0])["features"])[1] - 5
    trainer = train_rcnn.make_trainer(c, VF.IMG_CONV, seed=0)
    state = trainer.rng_state.clone()
    res = validate.validate_rcnn(dataset, out, trainer, "train", batch=3, workers=2)
    assert trainer.training and torch.equal(trainer.rng_state, state), "the val route must not touch the mode or the sampler's state"
    assert res["names"] == NAMES and res["batch_frames"] == [3, 1]
    trainer.eval()
    data = RD.KittiRcnnBatches(dataset, out, "train", mode="val", batch=3, workers=2)
    losses, correct = [], []
    try:
        with torch.no_grad():
            for bt in data:
                rois, iou, gt_of, _ = RT.proposal_targets(bt.proposals, bt.proposal_count, bt.gt, bt.gt_count, cfg=trainer.tcfg, train=False)
                assert torch.equal(rois, bt.proposals), "val: every proposal takes part"
                cls_logits, reg, pool = trainer.model(bt.xyz, bt.rpn_fts, bt.intensity, bt.fg_mask, rois, bt.image, bt.calib)
                flat_gt = gt_of.reshape(-1, 8)
                gt_cls = flat_gt[:, 7].to(torch.int32)
                loss, parts = RT.rcnn_loss_fused(trainer.model.cfg, trainer.tcfg, cls_logits, reg, iou.reshape(-1), gt_cls, pool["non_empty"],
                                                 RT.rcnn_encode(trainer.model.cfg, rois.reshape(-1, 7), flat_gt))
                losses.append([float(parts["box_classification"]), float(parts["bin_classification"]), float(parts["regression"]), float(loss)])
                target = torch.where(iou.reshape(-1) < trainer.tcfg.cls_neg_iou_range[1], torch.zeros_like(gt_cls), gt_cls)
                correct += (cls_logits.argmax(dim=-1) == target).view(len(bt.names), -1).sum(dim=1).tolist()
    finally:
        data.close()
        trainer.train()
    want, got = np.asarray(losses, np.float32), res["batch_losses"]
    print("\nper-batch losses %s\nthe test's %s\nlargest difference %g" % (got.tolist(), want.tolist(), np.abs(got - want).max()))
    assert np.isfinite(got).all() and (got > 0).all(), "a loss term without any RoI in its mask"
    assert np.array_equal(got, want), "the validation losses are not rcnn_loss_fused of the same batches, bit for bit"
    avg = (want.astype(np.float64) * np.array([[3.0], [1.0]])).sum(axis=0) / 4
    for k, v in zip(validate.RCNN_LOSSES, avg):
        assert res["totals"][k] == float(v), k
    assert res["rows"]["correct"].tolist() == correct and res["rows"]["rois"].tolist() == [100] * 4
    assert res["totals"]["cls_accuracy"] == sum(correct) / 400


def test_cli_over_a_checkpoint_directory(dataset, tmp_path):
    from heterofusionrcnn_amd import checkpoint, train_rpn
    ckpts, out = str(tmp_path / "ckpts"), str(tmp_path / "pred")
    train_rpn.train(dataset, "train", steps=2, batch=2, config="rpn_multiclass_points", log_every=0, workers=2, checkpoint_dir=ckpts,
                    checkpoint_every=1)
    assert [s for s, _ in checkpoint.list_checkpoints(ckpts)] == [1, 2]
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "heterofusionrcnn_amd.validate", "rpn", dataset, "--checkpoint-dir", ckpts,
           "--split", "train", "--config", "rpn_multiclass_points", "--batch", "3", "--workers", "2", "--out", out]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "2 checkpoints in" in r.stdout and "2 to evaluate" in r.stdout
    for step in (1, 2):
        assert "Step %d: Average RPN Losses: segmentation" % step in r.stdout
        assert "Step %d: Total RPN Recall@3DIoU=0.5:" % step in r.stdout
    files = sorted(os.listdir(out))
    assert files == ["rpn_avg_losses.csv", "rpn_avg_seg_acc.csv", "rpn_total_recall.csv"]
    before = {}
    for name, cols in zip(files, (5, 2, 7)):
        with open(os.path.join(out, name)) as f:
            before[name] = f.read()
        rows = [line.split(", ") for line in before[name].splitlines()]
        assert [row[0] for row in rows] == ["1", "2"] and all(len(row) == cols for row in rows), (name, rows)
        assert np.isfinite(np.array(rows, np.float64)).all()
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 to evaluate" in r.stdout and "Average RPN Losses" not in r.stdout
    for name in files:
        with open(os.path.join(out, name)) as f:
            assert f.read() == before[name], "%s changed on the second run" % name


def test_validation_leaves_no_worker_thread(dataset, handoff):
    """the reader threads (hf-read...) end with the call that started them"""
    from heterofusionrcnn_amd import rcnn_data as RD
    from heterofusionrcnn_amd import train_rcnn, validate
    workers = lambda: [t.name for t in threading.enumerate() if t.name.startswith(("hf-read", "hf-write"))]
    out, model_path, _ = handoff
    res = validate.validate_rpn(dataset, model_path, "train", batch=2, workers=2, img_conv=VF.IMG_CONV)
    assert res["names"] == NAMES and workers() == []
    c = RD.feature_shape(RD.handoff_paths(out, NAMES[0])["features"])[1] - 5
    res = validate.validate_rcnn(dataset, out, train_rcnn.make_trainer(c, VF.IMG_CONV, seed=0), "train", batch=2, workers=2)
    assert res["names"] == NAMES and workers() == []
