"""Export the RPN's hand-off for the second stage: python -m heterofusionrcnn_amd.export_rpn DATASET_DIR MODEL.pt OUT_DIR
[--split train] [--config rpn_multiclass] [--batch 8]

The reference's `run_inference.py --save_rpn_feature` (hf/core/evaluator.py:934-1065): the trained RPN runs in test mode over
every frame of the split, once, in order, without augmentation (kitti_data's device assembly: hf_rpn_batch_points,
hf_rpn_batch_image; the last batch may be short), and writes per frame
  OUT/proposals_and_scores/NAME.txt   every post_nms_size row (rpn_fixed_num_proposal_nms: the padded rows too), 7 box columns
                                      and the score, %.3f (kitti_io.save_proposals_and_scores)
  OUT/rpn_feature/NAME.npy            (P, 5 + c) float32 [x, y, z, intensity, fg, rpn_fts...] from hf_rpn_handoff_pack, one
                                      device-to-host copy per batch
  OUT/proposals_iou/NAME.txt          when label_2/NAME.txt exists: the (n, g) 3D IoU of the unrounded proposals x the labels of
                                      the configured classes (hf_box3d_iou_matrix), %.3f
and logs the reference's recall line per batch (Recall@3DIoU 0.5 / 0.7: the share of labels whose best proposal exceeds it).
Files are written by worker threads from pinned host buffers, so the device never waits on the disk.
"""
import argparse
import concurrent.futures
import contextlib
import os
import sys

import numpy as np
import torch

from . import checkpoint as ckpt_mod
from . import image_pyramid
from . import kitti_io
from . import kitti_data as KD
from .inference import CLASSES, rescale_p2
from .rcnn_data import HANDOFF_DIRS, box3d_iou_matrix, handoff_pack
from .train_rpn import CONFIGS, make_model


def read_export_frame(dataset_dir, name, classes, img_hw):
    """kitti_data.read_frame without augmentation; a frame without a label file has no boxes and no IoU file"""
    if os.path.isfile(os.path.join(dataset_dir, "label_2", name + ".txt")):
        fr = KD.read_frame(dataset_dir, name, (), classes, img_hw)
        fr["has_label"] = True
        return fr
    calib = kitti_io.read_calib(os.path.join(dataset_dir, "calib", name + ".txt"))
    image = KD.read_png(os.path.join(dataset_dir, "image_2", name + ".png"))
    h0, w0 = image.shape[:2]
    p2 = calib["p2"]
    return {"name": name, "augs": (), "points": kitti_io.read_velodyne(os.path.join(dataset_dir, "velodyne", name + ".bin")),
            "velo_to_rect": KD.velo_to_rect_matrix(calib), "p2": np.asarray(p2, np.float64), "wh": (w0, h0), "image": image,
            "flip": 0, "jitter": 0, "boxes": np.zeros((0, 7)), "cls": np.zeros((0,), np.int32), "has_label": False,
            "calib": rescale_p2(p2.astype(np.float32), (w0, h0), (img_hw[1], img_hw[0]))}


def recall_counts(iou):
    """(n, g) IoU -> (#labels with a proposal above 0.5, above 0.7) (box_util.compute_recall_iou)"""
    if iou.size == 0:
        return 0, 0
    best = iou.max(axis=0)
    return int((best > 0.5).sum()), int((best > 0.7).sum())


def _write_batch(out_dir, names, has_label, host, event, gcounts, batch_index, log):
    """worker thread: wait for the batch's copies, write its files, -> {name: totals}"""
    event.synchronize()
    rows, props, scores, iou = host["rows"].numpy(), host["proposals"].numpy(), host["scores"].numpy(), host["iou"].numpy()
    out, s50, s70, sl, sp = {}, 0, 0, 0, 0
    for i, name in enumerate(names):
        kitti_io.save_proposals_and_scores(os.path.join(out_dir, "proposals_and_scores", name + ".txt"), props[i], scores[i])
        np.save(os.path.join(out_dir, "rpn_feature", name + ".npy"), rows[i])
        tot = {"proposals": int(props.shape[1]), "labels": 0, "recall_50": 0, "recall_70": 0}
        if has_label[i]:
            m = iou[i, :, :gcounts[i]]
            np.savetxt(os.path.join(out_dir, "proposals_iou", name + ".txt"), m, fmt="%.3f")
            r50, r70 = recall_counts(m)
            tot.update(labels=int(gcounts[i]), recall_50=r50, recall_70=r70)
            s50, s70, sl = s50 + r50, s70 + r70, sl + int(gcounts[i])
        sp += tot["proposals"]
        out[name] = tot
    if log:
        log("Batch %d: RPN Recall@3DIoU=0.5: %.3f  Recall@3DIoU=0.7: %.3f, num proposals: %d" % (
            batch_index, s50 / max(sl, 1), s70 / max(sl, 1), sp))
    return out


class WriteBack:
    """Results on their way back to files without the device waiting for the disk: two sets of pinned host tensors used in
    turn (grown on demand), one non-blocking copy per tensor, an event behind the copies, and two writer threads.
    submit(dev, write, head, tail) copies `dev` (a device tensor, or a dict of them) and runs write(*head, host, event, *tail)
    -> dict on a writer thread (it waits for the event first); a set is reused only after its previous writer has returned.
    drain() -> every writer's dict, merged."""

    def __init__(self):
        self._writer = concurrent.futures.ThreadPoolExecutor(max_workers=2, thread_name_prefix="hf-write")
        self._sets, self._writes, self._turn, self._results = [{}, {}], [None, None], 0, {}

    def _collect(self, i):
        if self._writes[i] is not None:
            self._results.update(self._writes[i].result())

    def submit(self, dev, write, head, tail=()):
        single = torch.is_tensor(dev)
        dev = {"": dev} if single else dev
        i = self._turn
        self._turn ^= 1
        self._collect(i)                             # the pinned set of this parity is free once its last writer has finished
        hs = self._sets[i]
        for k, t in dev.items():
            if k not in hs or hs[k].numel() < t.numel():
                hs[k] = torch.empty((t.numel() * 5 // 4 + 1,), dtype=t.dtype).pin_memory()
        host = {k: hs[k][:t.numel()].view(t.shape) for k, t in dev.items()}
        for k, t in dev.items():
            host[k].copy_(t, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._writes[i] = self._writer.submit(write, *head, host[""] if single else host, done, *tail)

    def drain(self):
        self._collect(0)
        self._collect(1)
        return self._results

    def close(self):
        self._writer.shutdown(wait=True)


def load_rpn(model, config, img_conv):
    """a path to a saved state_dict or to a checkpoint, a state_dict, or a built model -> the model"""
    if isinstance(model, torch.nn.Module):
        return model
    sd = torch.load(model, map_location="cpu") if isinstance(model, (str, os.PathLike)) else model
    net, _ = make_model(config, img_conv)
    net.load_state_dict(ckpt_mod.model_state(sd), strict=True)
    return net


def proposals_from_files(net, dataset_dir, names, batch, workers, seed, num_points, img_hw, nms, classes, always_image=False):
    """File names -> the RPN's proposals, a generator over the chunks of `batch` names (the last may be short): frames are read
    one chunk ahead (kitti_data.ReadAhead) and packed on the caller's thread (measured: profiles/read_ahead_ab.md), then
    upload, hf_rpn_batch_points, geometry, hf_rpn_batch_image and propose(..., *nms) on the current stream; yields (frames,
    meta, xyz, intensity, image or None, the propose output).
    The image is drawn when the model has an image branch, from the [seed, call] pair of the points.  always_image: a
    points-only RPN gets one too (the RCNN needs it), its calls counted on a pair apart, so that the point samples stay those
    of a run without it (without jitter the image draws nothing).  Close the generator to stop the reader threads."""
    with_image = hasattr(net, "img_net")
    rpn = net.rpn if with_image else net
    device = next(net.parameters()).device
    rng_state = torch.tensor([int(seed), 0], dtype=torch.int64, device=device)
    img_rng = rng_state if with_image else torch.tensor([int(seed), 0], dtype=torch.int64, device=device)
    chunks = [names[i:i + batch] for i in range(0, len(names), batch)]

    def read(chunk, staging, pool):
        return list(pool.map(lambda n: read_export_frame(dataset_dir, n, list(classes), img_hw), chunk)), staging

    with KD.ReadAhead(read, workers) as feed:
        feed.submit(chunks[0] if chunks else None)
        for bi in range(len(chunks)):
            frames, staging = feed.take()          # the feeder has waited for this staging's event
            packed = KD.pack_frames(frames, staging)
            points, images, meta = KD.upload(packed, device)
            feed.uploaded()
            feed.submit(chunks[bi + 1] if bi + 1 < len(chunks) else None)
            xyz, inten, _, _ = KD.batch_points(points, meta["offsets"], meta["velo_to_rect"], meta["p2"], meta["wh"], meta["flip"],
                                               rng_state, num_points, packed["max_frame_points"])
            geo = rpn.geometry(xyz)
            image = KD.batch_image(images, meta["img_offsets"], meta["wh"], meta["flip"], meta["jitter"], img_rng, img_hw,
                                   packed["max_pixels"])[0] if with_image or always_image else None
            fts, calib = (net.img_net(image), meta["calib"]) if with_image else (None, None)
            yield frames, meta, xyz, inten, image, rpn.propose(xyz, inten, geo, fts, calib, *nms)


@torch.no_grad()
def export(dataset_dir, model, out_dir, split="train", config="rpn_multiclass", batch=8, img_conv=None, workers=8, seed=0,
           num_points=16384, img_hw=(360, 1200), pre_nms_size=9000, nms_thresh=0.8, post_nms_size=100, classes=CLASSES, log=print,
           image_branch="torch", image_precision="fp32"):
    """image_branch: image_pyramid.image_branch for the pyramid's calls; image_precision: image_pyramid.image_precision next to it
    ("bf16" needs image_branch="native": ValueError otherwise).
    model: a path to a saved state_dict (train_rpn --save) or to a checkpoint (train_rpn --checkpoint-dir), a state_dict, or a
    built model (RpnModel / RpnWithImageBranch).
    -> {name: {"proposals", "labels", "recall_50", "recall_70"}} for every frame of the split"""
    image_pyramid.check_precision_route(image_branch, image_precision)
    net = load_rpn(model, config, img_conv)
    was_training = net.training
    net.eval()
    names = KD.read_split(dataset_dir, split)
    for d in HANDOFF_DIRS:
        os.makedirs(os.path.join(out_dir, d), exist_ok=True)
    batches = proposals_from_files(net, dataset_dir, names, batch, workers, seed, num_points, img_hw,
                                   (pre_nms_size, nms_thresh, post_nms_size), classes)
    try:
        with image_pyramid.image_branch(image_branch), image_pyramid.image_precision(image_precision), contextlib.closing(batches), \
                contextlib.closing(WriteBack()) as back:
            for bi, (frames, meta, xyz, inten, _, out) in enumerate(batches):
                rows = handoff_pack(xyz, inten, out["fg_mask"], out["rpn_fts"])
                b, m = out["proposals"].shape[:2]
                gt = torch.cat([meta["boxes"], meta["cls"].unsqueeze(-1).float()], dim=-1)
                iou = box3d_iou_matrix(out["proposals"], torch.full((b,), m, dtype=torch.int32, device=xyz.device), gt, meta["gt_count"])
                back.submit({"rows": rows, "proposals": out["proposals"], "scores": out["proposal_scores"], "iou": iou}, _write_batch,
                            (out_dir, [f["name"] for f in frames], [f["has_label"] for f in frames]),
                            ([len(f["cls"]) for f in frames], bi, log))
            return back.drain()
    finally:
        net.train(was_training)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m heterofusionrcnn_amd.export_rpn",
                                 description="Run a trained RPN (train_rpn --save) over a split and write the second stage's "
                                             "training data: proposals_and_scores/, rpn_feature/ and proposals_iou/ under OUT_DIR.")
    ap.add_argument("dataset_dir")
    ap.add_argument("model", help="the state_dict saved by train_rpn --save, or a checkpoint file (ckpt-NNNNNNNN.pt)")
    ap.add_argument("out_dir")
    ap.add_argument("--split", default="train", help="a list file, or NAME for NAME.txt next to or inside DATASET_DIR")
    ap.add_argument("--config", choices=CONFIGS, default="rpn_multiclass")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0, help="seed of the point sampling")
    ap.add_argument("--workers", type=int, default=8, help="host threads that read and decode the files")
    ap.add_argument("--image-branch", choices=image_pyramid.IMAGE_BRANCHES, default="torch",
                    help="native: the VGG pyramid on this package's channel-last convolution kernels instead of the vendor library")
    ap.add_argument("--image-precision", choices=image_pyramid.IMAGE_PRECISIONS, default="fp32",
                    help="bf16: with --image-branch native, the pyramid's convolutions on the bf16 matrix cores (fp32 tensors and accumulation)")
    args = ap.parse_args(argv)
    if args.image_precision == "bf16" and args.image_branch != "native":
        ap.error("--image-precision bf16 needs --image-branch native")
    totals = export(args.dataset_dir, args.model, args.out_dir, args.split, args.config, args.batch, workers=args.workers,
                    seed=args.seed, image_branch=args.image_branch, image_precision=args.image_precision)
    labels = sum(t["labels"] for t in totals.values())
    print("done: %d frames, %d labels, Recall@3DIoU=0.5: %.3f  Recall@3DIoU=0.7: %.3f" % (
        len(totals), labels, sum(t["recall_50"] for t in totals.values()) / max(labels, 1),
        sum(t["recall_70"] for t in totals.values()) / max(labels, 1)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
