"""Detect from KITTI files with both trained models: python -m heterofusionrcnn_amd.detect DATASET_DIR RPN.pt RCNN.pt OUT_DIR
[--split val] [--config rpn_multiclass] [--batch 8] [--seed 0] [--workers 8] [--score-threshold 0.1] [--handoff-rounding]
[--host-rows] [--eval] [--precision {fp32,bf16}] [--image-branch {torch,native}] [--image-precision {fp32,bf16}]

The reference's `run_inference.py` over both stages (hf/core/evaluator.py:934-1065 for the first, :300-420 and
evaluator_utils.py:88-166 for the second), without the hand-off on disk: RPN.pt is what train_rpn --save (or a checkpoint of
it) holds, RCNN.pt what train_rcnn --save (or a checkpoint of it) holds, each with its own VGG pyramid; OUT_DIR/NAME.txt is a
KITTI result file for EVERY frame of the split (empty when nothing is kept; frames without labels included).

Per batch, on the device: the front half of export_rpn.export unchanged (read_export_frame one batch ahead, pack_frames,
upload, hf_rpn_batch_points, geometry, hf_rpn_batch_image, propose: equal --seed and --batch give the point samples an export
would have written), the in-memory hand-off (rcnn_data.handoff_in_memory; --handoff-rounding hands the proposals over with the
three decimals of the file route), RcnnWithImageBranch.detect on the SAME resized image (computed once; the file route's val
loader makes the same one: flip 0, jitter 0), then hf_kitti_result_boxes (inference.result_boxes) and one non-blocking copy
of the batch's rows to pinned host memory.  Worker threads format and write the files behind an event, so the device waits
neither for the disk nor for the text.  --host-rows keeps inference.write_frame_results (host projection, box by box) as
the writer: the parity anchor, byte-identical to rcnn_data.run_rcnn_from_handoff on an export with the same seed and batch.
--precision bf16 sends the wide dense layers of both stages to the bf16 matrix-core kernel (mlp.inference_precision; the heads that
are decoded into scores and boxes stay fp32); the default, fp32, is the route described above, bit for bit.
--image-branch native runs both VGG pyramids (the RPN's and the RCNN's) on the channel-last kernels of csrc/conv_nhwc.hip
(image_pyramid.image_branch); the default, torch, leaves them on the vendor library.
--image-precision bf16 (with --image-branch native only) runs their convolutions on csrc/conv_nhwc_bf16.hip (image_pyramid.image_precision).
"""
import argparse
import contextlib
import os
import sys

import numpy as np
import torch

from . import checkpoint as ckpt_mod
from . import image_pyramid
from . import kitti_data as KD
from . import mlp
from .export_rpn import WriteBack, load_rpn, proposals_from_files
from .inference import CLASSES, result_boxes, result_rows, write_frame_results, write_result_rows
from .rcnn_data import handoff_in_memory
from .rcnn_train import RcnnTrainer
from .train_rcnn import make_trainer
from .train_rpn import CONFIGS


def rpn_fts_channels(rpn):
    """the width of RpnModel.propose's rpn_fts: the backbone's output, plus the image channels under concat fusion"""
    return rpn.backbone.out_channel + (rpn.cfg.img_channels if rpn.cfg.fusion == "concat" else 0)


def load_models(rpn, rcnn, config="rpn_multiclass", img_conv=None):
    """rpn: a train_rpn --save file, a checkpoint of it, a state_dict or a built model (RpnModel / RpnWithImageBranch);
    rcnn: a train_rcnn --save file (the RcnnTrainer's state_dict), a checkpoint of it, a state_dict, an RcnnTrainer or an
    RcnnWithImageBranch.  Files and state_dicts load with strict=True; the RCNN is sized from the loaded RPN.
    -> (the RPN module, the RcnnWithImageBranch)"""
    net = load_rpn(rpn, config, img_conv)
    if isinstance(rcnn, torch.nn.Module):
        second = rcnn.model if isinstance(rcnn, RcnnTrainer) else rcnn
    else:
        trainer = make_trainer(rpn_fts_channels(net.rpn if hasattr(net, "img_net") else net), img_conv)
        sd = torch.load(rcnn, map_location="cpu") if isinstance(rcnn, (str, os.PathLike)) else rcnn
        trainer.load_state_dict(ckpt_mod.model_state(sd), strict=True)
        second = trainer.model
    return net, second


def _write_rows(out_dir, names, counts, host, event, classes):
    """worker thread: wait for the batch's copy, write its files from the device rows -> {name: rows written}"""
    event.synchronize()
    rows = host.numpy()
    out, at = {}, 0
    for name, n in zip(names, counts):
        out[name] = write_result_rows(os.path.join(out_dir, name + ".txt"), rows[at:at + n], classes)
        at += n
    return out


@torch.no_grad()
def detect(dataset_dir, rpn, rcnn, out_dir, split="val", config="rpn_multiclass", batch=8, seed=0, workers=8, score_threshold=0.1,
           handoff_rounding=False, host_rows=False, img_conv=None, num_points=16384, img_hw=(360, 1200), pre_nms_size=9000,
           nms_thresh=0.8, post_nms_size=100, classes=CLASSES, precision="fp32", image_branch="torch", image_precision="fp32"):
    """rpn / rcnn: see load_models.  precision: mlp.inference_precision for the duration of the call; image_branch:
    image_pyramid.image_branch for the same duration, over both pyramids; image_precision: image_pyramid.image_precision next to it
    ("bf16" needs image_branch="native": ValueError otherwise).
    -> {name: rows written} for every frame of the split"""
    image_pyramid.check_precision_route(image_branch, image_precision)
    scope, img_scope = mlp.inference_precision(precision), image_pyramid.image_branch(image_branch)
    img_prec = image_pyramid.image_precision(image_precision)
    net, second = load_models(rpn, rcnn, config, img_conv)
    modes = (net.training, second.training)
    net.eval()
    second.eval()
    names = KD.read_split(dataset_dir, split)
    os.makedirs(out_dir, exist_ok=True)
    batches = proposals_from_files(net, dataset_dir, names, batch, workers, seed, num_points, img_hw,
                                   (pre_nms_size, nms_thresh, post_nms_size), classes, always_image=True)
    written = {}
    try:
        with scope, img_scope, img_prec, contextlib.closing(batches), contextlib.closing(WriteBack()) as back:
            for frames, meta, xyz, inten, image, out in batches:
                h = handoff_in_memory(out, xyz, inten, handoff_rounding)
                dets, _ = second.detect(h["xyz"], h["rpn_fts"], h["intensity"], h["fg_mask"], h["proposals"], image, meta["calib"])
                if host_rows:
                    for f, det in zip(frames, dets):
                        written[f["name"]] = write_frame_results(os.path.join(out_dir, f["name"] + ".txt"), det,
                                                                 np.asarray(f["p2"], np.float32), f["wh"], score_threshold, classes)
                    continue
                res = result_boxes(dets, meta["p2"], meta["wh"], score_threshold)
                back.submit(result_rows(res), _write_rows, (out_dir, [f["name"] for f in frames], res["counts"]), (classes,))
            written.update(back.drain())
    finally:
        net.train(modes[0])
        second.train(modes[1])
    return written


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m heterofusionrcnn_amd.detect",
                                 description="Run a trained RPN (train_rpn --save) and a trained RCNN (train_rcnn --save) over a "
                                             "split and write one KITTI result file per frame to OUT_DIR.")
    ap.add_argument("dataset_dir")
    ap.add_argument("rpn", help="the state_dict saved by train_rpn --save, or a checkpoint file (ckpt-NNNNNNNN.pt)")
    ap.add_argument("rcnn", help="the state_dict saved by train_rcnn --save, or a checkpoint file")
    ap.add_argument("out_dir")
    ap.add_argument("--split", default="val", help="a list file, or NAME for NAME.txt next to or inside DATASET_DIR")
    ap.add_argument("--config", choices=CONFIGS, default="rpn_multiclass", help="the RPN's config")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0, help="seed of the point sampling")
    ap.add_argument("--workers", type=int, default=8, help="host threads that read and decode the files")
    ap.add_argument("--score-threshold", type=float, default=0.1)
    ap.add_argument("--handoff-rounding", action="store_true",
                    help="hand the proposals over with three decimals, as the on-disk hand-off does")
    ap.add_argument("--host-rows", action="store_true", help="project and filter the boxes on the host (write_frame_results)")
    ap.add_argument("--eval", action="store_true", help="then evaluate OUT_DIR against DATASET_DIR/label_2 (kitti_eval)")
    ap.add_argument("--precision", choices=mlp.PRECISIONS, default="fp32",
                    help="bf16: the wide dense layers of both stages on the bf16 matrix cores (fp32 accumulation, fp32 output heads)")
    ap.add_argument("--image-branch", choices=image_pyramid.IMAGE_BRANCHES, default="torch",
                    help="native: both VGG pyramids on this package's channel-last convolution kernels instead of the vendor library")
    ap.add_argument("--image-precision", choices=image_pyramid.IMAGE_PRECISIONS, default="fp32",
                    help="bf16: with --image-branch native, the pyramid's convolutions on the bf16 matrix cores (fp32 tensors and accumulation)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.image_precision == "bf16" and args.image_branch != "native":
        ap.error("--image-precision bf16 needs --image-branch native")
    written = detect(args.dataset_dir, args.rpn, args.rcnn, args.out_dir, args.split, args.config, args.batch, args.seed,
                     args.workers, args.score_threshold, args.handoff_rounding, args.host_rows, precision=args.precision,
                     image_branch=args.image_branch, image_precision=args.image_precision)
    print("done: %d frames, %d rows" % (len(written), sum(written.values())))
    if args.eval:
        from . import kitti_eval
        return kitti_eval.main([os.path.join(args.dataset_dir, "label_2"), args.out_dir])
    return 0


if __name__ == "__main__":
    sys.exit(main())
