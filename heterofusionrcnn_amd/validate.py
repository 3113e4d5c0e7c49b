"""Validate trained checkpoints on a split:
  python -m heterofusionrcnn_amd.validate rpn  DATASET_DIR (MODEL.pt | --checkpoint-dir DIR) [--split val] [--out DIR] [--batch N]
  python -m heterofusionrcnn_amd.validate rcnn DATASET_DIR HANDOFF_DIR (MODEL.pt | --checkpoint-dir DIR) [--split val] [--out DIR]

The reference's `run_evaluation.py` (hf/core/evaluator.py:149-377 run_checkpoint_once, :379-433 run_latest_checkpoints): the model
runs in evaluation mode over every frame of the split, once, in order, without augmentation; the losses, the segmentation
(RPN) or box-classification (RCNN) accuracy and the RPN's proposal statistics (recall at 3D IoU 0.5 / 0.7, mean BEV and 3D IoU
of the proposals, mean angle residual: :984-1064, hf/core/box_util.py:131-174) are accumulated, the reference's summary lines
printed and, with --out, one row per evaluated model appended to
  rpn_avg_losses.csv  rpn_avg_seg_acc.csv  rpn_total_recall.csv        (save_rpn_stats, :623-724)
  rcnn_avg_losses.csv  rcnn_avg_cls_acc.csv                           (save_prediction_stats, :726-797)
whose first column is the checkpoint's global step (a bare --save file: 0).  --checkpoint-dir evaluates every checkpoint of the
directory in ascending order and skips a step already in the first column of the stage's losses file (get_evaluated_ckpts,
:835-872).  Result files and AP stay with `detect --eval`.

Everything per frame is computed on the device (csrc/eval_stats.hip: hf_proposal_stats, hf_argmax_accuracy; the fused loss
forwards; kitti_data.point_labels; rcnn_train.proposal_targets(train=False)) into tables sized for the split, which the host
reads once at the end: nothing synchronises per batch.

Two definitions differ from the reference, which sums a per-batch value and divides by the sample count (:642-646) -- the same
thing at its batch size of 1:
  accuracy        correct points (RoIs) / points (RoIs) of the split;
  average losses  the per-batch losses weighted by the frames in the batch (the last batch may be short).
And one in hf_proposal_stats: a frame without labels adds 0 to the angle-residual sum (the reference adds sum |ry|).
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

from . import _lib
from . import checkpoint as ckpt_mod
from . import image_pyramid
from . import kitti_data as KD
from ._lib import check, dev_tensor, ptr, require, stream_ptr
from .inference import CLASSES

RPN_LOSSES = ("segmentation", "bin_classification", "regression", "total")
RCNN_LOSSES = ("box_classification", "bin_classification", "regression", "total")
# file name -> (fmt, the totals' keys after the step); column order and fmt of evaluator.py:682-724 and :773-797 (the last
# column of rpn_avg_losses.csv is "%5f" there: six decimals)
RPN_CSV = {
    "rpn_avg_losses.csv": ("%d, %.5f, %.5f, %.5f, %5f", RPN_LOSSES),
    "rpn_avg_seg_acc.csv": ("%d, %.5f", ("seg_accuracy",)),
    "rpn_total_recall.csv": ("%d, %.5f, %.5f, %.5f, %.5f, %.5f, %.5f",
                             ("recall_50", "recall_70", "avg_proposals", "iou_2d", "iou_3d", "angle_residual")),
}
RCNN_CSV = {
    "rcnn_avg_losses.csv": ("%d, %.5f, %.5f, %.5f, %.5f", RCNN_LOSSES),
    "rcnn_avg_cls_acc.csv": ("%d, %.5f", ("cls_accuracy",)),
}
STAGES = {"rpn": (RPN_CSV, "rpn_avg_losses.csv"), "rcnn": (RCNN_CSV, "rcnn_avg_losses.csv")}


# ------------------------------------------------------------------------------------------------ device calls
def proposal_stats(proposals, proposal_count, gt, gt_count, counts=None, sums=None, matrices=False):
    """hf_proposal_stats: proposals (B,m,7), gt (B,g,8) [box, cls], counts (B,) int32 -> dict with best_iou3d, best_iou2d (B,m),
    best_gt (B,m) int32, counts (B,4) int32 [proposals, labels, recalled at 0.5, at 0.7], sums (B,3) fp64 [sum best_iou2d, sum
    best_iou3d, sum |ry - ry of the best GT|]; matrices=True adds iou3d and iou2d (B,m,g).  counts / sums: contiguous views to
    write into (rows of a table sized for the whole split)."""
    require(proposals.dim() == 3 and proposals.shape[2] == 7, "proposals must be (B, m, 7)")
    require(gt.dim() == 3 and gt.shape[2] == 8 and gt.shape[0] == proposals.shape[0], "gt must be (B, g, 8)")
    b, m, _ = proposals.shape
    g = gt.shape[1]
    props = dev_tensor(proposals.detach(), torch.float32, "proposals")
    gts = dev_tensor(gt.detach(), torch.float32, "gt")
    pc = dev_tensor(proposal_count, torch.int32, "proposal_count")
    gc = dev_tensor(gt_count, torch.int32, "gt_count")
    require(pc.numel() == b and gc.numel() == b, "counts must be (B,)")
    dev = props.device
    counts = torch.empty((b, 4), dtype=torch.int32, device=dev) if counts is None else counts
    sums = torch.empty((b, 3), dtype=torch.float64, device=dev) if sums is None else sums
    require(counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == (b, 4) and counts.is_contiguous(),
            "counts must be a contiguous (B, 4) int32 device tensor")
    require(sums.is_cuda and sums.dtype == torch.float64 and tuple(sums.shape) == (b, 3) and sums.is_contiguous(),
            "sums must be a contiguous (B, 3) float64 device tensor")
    out = {"best_iou3d": torch.empty((b, m), dtype=torch.float32, device=dev),
           "best_iou2d": torch.empty((b, m), dtype=torch.float32, device=dev),
           "best_gt": torch.empty((b, m), dtype=torch.int32, device=dev), "counts": counts, "sums": sums}
    if matrices:
        out["iou3d"] = torch.empty((b, m, g), dtype=torch.float32, device=dev)
        out["iou2d"] = torch.empty((b, m, g), dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = L.hf_proposal_stats_workspace(b, m, g)
    ws = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=dev)
    check(L.hf_proposal_stats(b, m, g, ptr(props), ptr(pc), ptr(gts) if g > 0 else None, ptr(gc), ptr(out.get("iou3d")),
                              ptr(out.get("iou2d")), ptr(out["best_iou3d"]), ptr(out["best_iou2d"]), ptr(out["best_gt"]), ptr(counts),
                              ptr(sums), ptr(ws), int(nbytes), stream_ptr()), "proposal_stats")
    return out


def argmax_accuracy(logits, target, groups=1, out=None):
    """hf_argmax_accuracy: logits (rows, c) float32, target (rows,) int32 -> correct (groups,) int32: per group of rows / groups
    consecutive rows, the rows whose first argmax equals max(target, 0).  out: a contiguous (groups,) int32 view to write into."""
    require(logits.dim() == 2 and target.dim() == 1 and target.numel() == logits.shape[0], "logits must be (rows, c), target (rows,)")
    rows, c = logits.shape
    lg = dev_tensor(logits.detach(), torch.float32, "logits")
    tg = dev_tensor(target, torch.int32, "target")
    out = torch.empty((int(groups),), dtype=torch.int32, device=lg.device) if out is None else out
    require(out.is_cuda and out.dtype == torch.int32 and out.numel() == int(groups) and out.is_contiguous(),
            "out must be a contiguous (groups,) int32 device tensor")
    check(_lib.lib().hf_argmax_accuracy(rows, c, int(groups), ptr(lg), ptr(tg), ptr(out), stream_ptr()), "argmax_accuracy")
    return out


# ------------------------------------------------------------------------------------------------ host arithmetic
def frame_weighted_losses(batch_losses, batch_frames, keys):
    """per-batch losses (nb, len(keys)) and the frames of each batch -> {key: sum(loss_b * frames_b) / frames} in fp64"""
    losses = np.asarray(batch_losses, np.float64).reshape(len(batch_frames), len(keys))
    w = np.asarray(batch_frames, np.float64)
    avg = (losses * w[:, None]).sum(axis=0) / max(w.sum(), 1.0)
    return {k: float(v) for k, v in zip(keys, avg)}


def rpn_totals(rows, batch_losses, batch_frames):
    """the totals of save_rpn_stats (evaluator.py:623-679) from the per-frame rows (a dict of equally long arrays: proposals,
    labels, recall_50, recall_70, sum_iou2d, sum_iou3d, sum_angle, correct, points) and the per-batch losses"""
    s = {k: np.asarray(v).sum() for k, v in rows.items()}
    frames = len(rows["proposals"])
    labels, props = max(int(s["labels"]), 1), max(int(s["proposals"]), 1)
    tot = frame_weighted_losses(batch_losses, batch_frames, RPN_LOSSES)
    tot.update(frames=frames, labels=int(s["labels"]), seg_accuracy=float(s["correct"]) / max(int(s["points"]), 1),
               recall_50=float(s["recall_50"]) / labels, recall_70=float(s["recall_70"]) / labels,
               avg_proposals=float(s["proposals"]) / max(frames, 1), iou_2d=float(s["sum_iou2d"]) / props,
               iou_3d=float(s["sum_iou3d"]) / props, angle_residual=float(s["sum_angle"]) / props)
    return tot


def rcnn_totals(rows, batch_losses, batch_frames):
    """the totals of save_prediction_stats (evaluator.py:726-770) from the per-frame rows (correct, rois) and the per-batch losses"""
    tot = frame_weighted_losses(batch_losses, batch_frames, RCNN_LOSSES)
    tot.update(frames=len(rows["rois"]), cls_accuracy=float(np.asarray(rows["correct"]).sum()) / max(int(np.asarray(rows["rois"]).sum()), 1))
    return tot


def summary_lines(stage, step, tot):
    """the reference's summary lines (evaluator.py:655-679, :752-770)"""
    if stage == "rpn":
        return ["Step {}: Average RPN Losses: segmentation {:.3f}, bin_cls {:.3f}, regression {:.3f}, total {:.3f}".format(
                    step, tot["segmentation"], tot["bin_classification"], tot["regression"], tot["total"]),
                "Step {}: Average Segmentation Accuracy:{:.3f} ".format(step, tot["seg_accuracy"]),
                "Step {}: Total RPN Recall@3DIoU=0.5: {:.3f}  Recall@3DIoU=0.7: {:.3f}, Average Proposals: {:.3f}".format(
                    step, tot["recall_50"], tot["recall_70"], tot["avg_proposals"]),
                "Step {}: Average RPN IoU_2D: {:.3f} , IoU_3D: {:.3f}, Average Angel Residual: {:.3f}".format(
                    step, tot["iou_2d"], tot["iou_3d"], tot["angle_residual"])]
    return ["Step {}: Average RCNN Losses: cls {:.5f}, bin_cls {:.5f}, reg {:.5f}, total {:.5f} ".format(
                step, tot["box_classification"], tot["bin_classification"], tot["regression"], tot["total"]),
            "Step {}: Average Classification Accuracy: {:.3f} ".format(step, tot["cls_accuracy"])]


def append_csv(out_dir, stage, step, tot):
    """one row per file of the stage, appended (np.savetxt's line: fmt % the row, then a newline)"""
    os.makedirs(out_dir, exist_ok=True)
    for name, (fmt, keys) in STAGES[stage][0].items():
        with open(os.path.join(out_dir, name), "a") as f:
            f.write(fmt % ((int(step),) + tuple(float(tot[k]) for k in keys)) + "\n")


def evaluated_steps(out_dir, stage):
    """the global steps in the first column of the stage's losses file (get_evaluated_ckpts); no file: none"""
    path = os.path.join(out_dir, STAGES[stage][1]) if out_dir else None
    if not path or not os.path.exists(path):
        return set()
    with open(path) as f:
        return {int(float(line.split(",")[0])) for line in f if line.strip()}


def pending_checkpoints(found, done):
    """[(step, path)] of checkpoint.list_checkpoints, ascending, without the steps already evaluated"""
    return [(int(s), p) for s, p in sorted(found) if int(s) not in done]


def global_step_of(path):
    """the global step a model file stands for: a checkpoint's, 0 for a bare --save state_dict"""
    sd = torch.load(path, map_location="cpu")
    return int(sd["global_step"]) if ckpt_mod.is_checkpoint(sd) else 0


# ------------------------------------------------------------------------------------------------ the RPN
@torch.no_grad()
def validate_rpn(dataset_dir, model, split="val", config="rpn_multiclass", batch=8, seed=0, workers=8, img_conv=None,
                 num_points=16384, img_hw=(360, 1200), pre_nms_size=9000, nms_thresh=0.8, post_nms_size=100, classes=CLASSES,
                 image_branch="torch", image_precision="fp32"):
    """image_branch: image_pyramid.image_branch for the pyramid's calls; image_precision: image_pyramid.image_precision next to it
    ("bf16" needs image_branch="native": ValueError otherwise).
    model: whatever export_rpn.load_rpn accepts (a --save file, a checkpoint file, a state_dict, a built model).  The frames
    of the split are read once, in order, without augmentation (export_rpn.proposals_from_files: the point samples of
    export_rpn.export at the same seed); ONE eval-mode forward per batch (RpnModel.propose) feeds the fused loss forward
    (labels from kitti_data.point_labels), hf_argmax_accuracy and hf_proposal_stats.
    -> {"names", "frames": {name: {proposals, labels, recall_50, recall_70, sum_iou2d, sum_iou3d, sum_angle, correct, points}},
        "rows": the same as arrays in split order, "batch_losses" (nb, 4) [segmentation, bin_classification, regression, total],
        "batch_frames", "totals": rpn_totals(...)}
    Differences from the reference (evaluator.py:642-646 divides per-batch sums by the sample count; equal at its batch size 1):
    accuracy is correct points / points, and the average losses are the per-batch losses weighted by the frames in the batch."""
    from .export_rpn import load_rpn, proposals_from_files
    image_pyramid.check_precision_route(image_branch, image_precision)
    net = load_rpn(model, config, img_conv)
    rpn = net.rpn if hasattr(net, "img_net") else net
    was_training = net.training
    net.eval()
    names = KD.read_split(dataset_dir, split)
    n = len(names)
    dev = next(net.parameters()).device
    nb = (n + batch - 1) // batch
    counts = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    sums = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    correct = torch.zeros((n,), dtype=torch.int32, device=dev)
    losses = torch.zeros((nb, 4), dtype=torch.float32, device=dev)
    batch_frames, seen, points = [], [], 0
    batches = proposals_from_files(net, dataset_dir, names, batch, workers, seed, num_points, img_hw,
                                   (pre_nms_size, nms_thresh, post_nms_size), classes)
    try:
        with image_pyramid.image_branch(image_branch), image_pyramid.image_precision(image_precision), contextlib.closing(batches):
            for bi, (frames, meta, xyz, inten, _, out) in enumerate(batches):
                b, p = xyz.shape[:2]
                off = len(seen)
                label_cls, label_reg = KD.point_labels(xyz, meta["boxes"], meta["cls"], meta["gt_count"])
                loss, parts = rpn.loss(xyz, out["seg_logits"], out["head"], label_cls, label_reg)
                losses[bi] = torch.stack([parts["segmentation"], parts["bin_classification"], parts["regression"], loss.detach()])
                seg = out["seg_logits"]
                argmax_accuracy(seg.reshape(b * p, seg.shape[-1]), label_cls.reshape(-1), b, correct[off:off + b])
                m = out["proposals"].shape[1]
                gt = torch.cat([meta["boxes"], meta["cls"].unsqueeze(-1).float()], dim=-1)
                proposal_stats(out["proposals"], torch.full((b,), m, dtype=torch.int32, device=dev), gt, meta["gt_count"],
                               counts[off:off + b], sums[off:off + b])
                seen += [f["name"] for f in frames]
                batch_frames.append(b)
                points = p
    finally:
        net.train(was_training)
    c, s, ok, ls = counts.cpu().numpy(), sums.cpu().numpy(), correct.cpu().numpy(), losses.cpu().numpy()   # the one read
    rows = {"proposals": c[:, 0], "labels": c[:, 1], "recall_50": c[:, 2], "recall_70": c[:, 3], "sum_iou2d": s[:, 0],
            "sum_iou3d": s[:, 1], "sum_angle": s[:, 2], "correct": ok, "points": np.full((n,), points, np.int64)}
    per_frame = {name: {k: v[i].item() for k, v in rows.items()} for i, name in enumerate(seen)}
    return {"names": seen, "frames": per_frame, "rows": rows, "batch_losses": ls, "batch_frames": batch_frames,
            "totals": rpn_totals(rows, ls, batch_frames)}


# ------------------------------------------------------------------------------------------------ the RCNN
def load_rcnn(model, rpn_fts_channels, img_conv=None):
    """a path to a saved RcnnTrainer state_dict (train_rcnn --save) or to a checkpoint, a state_dict, or a built RcnnTrainer
    -> the trainer"""
    from .rcnn_train import RcnnTrainer
    from .train_rcnn import make_trainer
    if isinstance(model, RcnnTrainer):
        return model
    sd = torch.load(model, map_location="cpu") if isinstance(model, (str, os.PathLike)) else model
    trainer = make_trainer(rpn_fts_channels, img_conv)
    trainer.load_state_dict(ckpt_mod.model_state(sd), strict=True)
    return trainer


def rcnn_val_forward(trainer, bt):
    """The val route of rcnn_train.RcnnTrainer for one rcnn_data.RcnnBatch (evaluator.py with kitti_dataset.py:509-513): every
    proposal with its max IoU and argmax GT (proposal_targets(train=False)), the model as it stands (call it in eval mode: no path
    drop), the fused loss forward.  -> (out6-style parts with "total", cls_logits (B m, K+1), target (B m,) int32: the
    box-classification label where(iou < cls_neg_hi, 0, gt class), rcnn_model.py:783-801)"""
    from .rcnn_train import proposal_targets, rcnn_encode, rcnn_loss_fused
    model, tcfg = trainer.model, trainer.tcfg
    rois, iou, gt_of, _ = proposal_targets(bt.proposals, bt.proposal_count, bt.gt, bt.gt_count, cfg=tcfg, train=False)
    cls_logits, reg, pool = model(bt.xyz, bt.rpn_fts, bt.intensity, bt.fg_mask, rois, bt.image, bt.calib)
    flat_rois, flat_gt = rois.reshape(-1, 7), gt_of.reshape(-1, 8)
    gt_cls = flat_gt[:, 7].to(torch.int32)
    loss, parts = rcnn_loss_fused(model.cfg, tcfg, cls_logits, reg, iou.reshape(-1), gt_cls, pool["non_empty"],
                                  rcnn_encode(model.cfg, flat_rois, flat_gt))
    parts = dict(parts, total=loss.detach())
    target = torch.where(iou.reshape(-1) < tcfg.cls_neg_iou_range[1], torch.zeros_like(gt_cls), gt_cls)
    return parts, cls_logits, target


@torch.no_grad()
def validate_rcnn(dataset_dir, handoff_dir, model, split="val", batch=2, workers=8, img_conv=None, image_branch="torch",
                  image_precision="fp32"):
    """image_branch: image_pyramid.image_branch for the pyramid's calls; image_precision: image_pyramid.image_precision next to it
    ("bf16" needs image_branch="native": ValueError otherwise).
    model: a train_rcnn --save file, a checkpoint file, a state_dict or a built rcnn_train.RcnnTrainer.  Frames with a label of
    the classes, once, in order, without augmentation (rcnn_data.KittiRcnnBatches(mode="val")); per batch rcnn_val_forward and
    hf_argmax_accuracy over the B m RoIs, one group per frame (padded proposal rows count as background RoIs).
    -> {"names", "frames": {name: {correct, rois}}, "rows", "batch_losses" (nb, 4) [box_classification, bin_classification,
        regression, total], "batch_frames", "totals": rcnn_totals(...)}
    Accuracy and average losses are defined as in validate_rpn (correct RoIs / RoIs; frame-weighted batch losses)."""
    from .rcnn_data import KittiRcnnBatches
    from .rcnn_train import RcnnTrainer
    image_pyramid.check_precision_route(image_branch, image_precision)
    device = next(model.parameters()).device if isinstance(model, RcnnTrainer) else None
    data = KittiRcnnBatches(dataset_dir, handoff_dir, split, mode="val", batch=batch, workers=workers, device=device)
    trainer, was_training = None, False
    try:
        trainer = load_rcnn(model, data.channels, img_conv)
        was_training = trainer.training
        trainer.eval()
        n, m = len(data), data.num_proposals
        nb = (n + batch - 1) // batch
        correct = torch.zeros((n,), dtype=torch.int32, device=data.device)
        losses = torch.zeros((nb, 4), dtype=torch.float32, device=data.device)
        batch_frames, seen = [], []
        for bi, bt in enumerate(data):
            b, off = len(bt.names), len(seen)
            with image_pyramid.image_branch(image_branch), image_pyramid.image_precision(image_precision):
                parts, cls_logits, target = rcnn_val_forward(trainer, bt)
            losses[bi] = torch.stack([parts[k] for k in RCNN_LOSSES])
            argmax_accuracy(cls_logits, target, b, correct[off:off + b])
            seen += list(bt.names)
            batch_frames.append(b)
    finally:
        data.close()
        if trainer is not None:
            trainer.train(was_training)
    ok, ls = correct.cpu().numpy(), losses.cpu().numpy()
    rows = {"correct": ok, "rois": np.full((n,), m, np.int64)}
    per_frame = {name: {k: v[i].item() for k, v in rows.items()} for i, name in enumerate(seen)}
    return {"names": seen, "frames": per_frame, "rows": rows, "batch_losses": ls, "batch_frames": batch_frames,
            "totals": rcnn_totals(rows, ls, batch_frames)}


# ------------------------------------------------------------------------------------------------ command line
def build_parser():
    from .train_rpn import CONFIGS
    ap = argparse.ArgumentParser(prog="python -m heterofusionrcnn_amd.validate",
                                 description="Run trained models over a split in evaluation mode: average losses, accuracy and (RPN) "
                                             "proposal recall / IoU, one CSV row per model with --out.")
    sub = ap.add_subparsers(dest="stage", required=True)
    for stage in ("rpn", "rcnn"):
        sp = sub.add_parser(stage)
        sp.add_argument("dataset_dir")
        if stage == "rcnn":
            sp.add_argument("handoff_dir", help="what export_rpn wrote for the split")
        sp.add_argument("model", nargs="?", default=None, help="a --save state_dict or a checkpoint file (ckpt-NNNNNNNN.pt)")
        sp.add_argument("--checkpoint-dir", default=None, help="evaluate every checkpoint of this directory not yet in --out")
        sp.add_argument("--split", default="val", help="a list file, or NAME for NAME.txt next to or inside DATASET_DIR")
        sp.add_argument("--out", default=None, help="directory of the CSV files (appended to)")
        sp.add_argument("--batch", type=int, default=8 if stage == "rpn" else 2)
        sp.add_argument("--workers", type=int, default=8, help="host threads that read and decode the files")
        if stage == "rpn":
            sp.add_argument("--config", choices=CONFIGS, default="rpn_multiclass")
            sp.add_argument("--seed", type=int, default=0, help="seed of the point sampling")
        sp.add_argument("--image-branch", choices=image_pyramid.IMAGE_BRANCHES, default="torch",
                        help="native: the VGG pyramid on this package's channel-last convolution kernels instead of the vendor library")
        sp.add_argument("--image-precision", choices=image_pyramid.IMAGE_PRECISIONS, default="fp32",
                        help="bf16: with --image-branch native, the pyramid's convolutions on the bf16 matrix cores (fp32 tensors and accumulation)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.image_precision == "bf16" and args.image_branch != "native":
        ap.error("--image-precision bf16 needs --image-branch native")
    if (args.model is None) == (args.checkpoint_dir is None):
        ap.error("give either MODEL.pt or --checkpoint-dir")
    if args.checkpoint_dir is not None:
        found = ckpt_mod.list_checkpoints(args.checkpoint_dir)
        todo = pending_checkpoints(found, evaluated_steps(args.out, args.stage))
        print("%d checkpoints in %s, %d to evaluate" % (len(found), args.checkpoint_dir, len(todo)))
    else:
        todo = [(global_step_of(args.model), args.model)]
    for step, path in todo:
        if args.stage == "rpn":
            res = validate_rpn(args.dataset_dir, path, args.split, args.config, args.batch, args.seed, args.workers,
                               image_branch=args.image_branch, image_precision=args.image_precision)
        else:
            res = validate_rcnn(args.dataset_dir, args.handoff_dir, path, args.split, args.batch, args.workers,
                                image_branch=args.image_branch, image_precision=args.image_precision)
        for line in summary_lines(args.stage, step, res["totals"]):
            print(line)
        if args.out:
            append_csv(args.out, args.stage, step, res["totals"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
