"""Train the RPN from KITTI files: python -m heterofusionrcnn_amd.train_rpn DATASET_DIR [--split train] [--steps N] ...

Batches come from kitti_data.KittiRpnBatches (device batch assembly, one batch ahead); the step is graph_step.TrainStep
(replayed from a captured hipGraph), with the geometry of the next batch prefetched on a side stream.  Configs that fuse the
image train RpnWithImageBranch(model, ImgVggPyr()), the reference's whole step.  --save writes the model's state_dict.

--reference-train-op runs the reference's train op (rpn_multiclass.config:204-224 train_config, hf/core/trainer.py:68-84):
Adam with TensorFlow's epsilon, per-tensor gradient clipping at 1.0 and a staircase exponential decay (0.001 x world, 20 000
steps, factor 0.8); a NaN / Inf loss then stops the run (check_numerics).  --checkpoint-dir writes a checkpoint (model,
optimizer, global step, dropout counters, generator states, loader position: checkpoint.py) every --checkpoint-every steps,
and --resume continues from the newest one up to the global step --steps.
"""
import argparse
import math
import sys
import time

import torch

from . import checkpoint as ckpt_mod
from . import rpn as rpn_mod
from .graph_step import TrainStep
from .inference import CLASSES, ImgVggPyr
from .kitti_data import KittiRpnBatches
from .mlp import under_training_precision
from .optim import MultiTensorAdam
from .pipeline import GeometryPrefetcher

CONFIGS = ("rpn_multiclass", "rpn_multiclass_points")


def make_model(config, img_conv=None):
    """rpn_multiclass: PointCNN RPN + image fusion + the VGG pyramid (img_conv: its (layers, channels) per level);
    rpn_multiclass_points: the same RPN without the image branch"""
    if config == "rpn_multiclass":
        img_net = ImgVggPyr(img_conv) if img_conv else ImgVggPyr()
        return rpn_mod.RpnWithImageBranch(rpn_mod.RpnModel(rpn_mod.rpn_multiclass(img_net.out_channel)), img_net).cuda(), True
    if config == "rpn_multiclass_points":
        return rpn_mod.RpnModel(rpn_mod.rpn_multiclass(0)).cuda(), False
    raise ValueError("config must be one of %s" % (CONFIGS,))


@under_training_precision
def train(dataset_dir, split="train", steps=100, batch=8, config="rpn_multiclass", seed=0, save=None, log_every=10, workers=8,
          lr=1e-3, graph=True, img_conv=None, num_points=16384, log=print, clip_norm=0.0, lr_decay=None, tf_epsilon=False,
          check_numerics=False, checkpoint_dir=None, checkpoint_every=ckpt_mod.CHECKPOINT_INTERVAL, max_checkpoints=None, resume=False,
          precision="fp32"):
    """-> (list of the per-step losses of this run, floats read at the end; the loader status)

    clip_norm / lr_decay / tf_epsilon: optim.MultiTensorAdam's (ckpt_mod.reference_train_op() holds the reference's values);
    check_numerics: a NaN / Inf loss raises FloatingPointError at the next log point (always before a checkpoint is written);
    checkpoint_dir: a checkpoint every checkpoint_every global steps, the newest max_checkpoints kept; resume: continue from the
    newest checkpoint there, `steps` then being the final global step.  precision "bf16": the wide dense layers train on the bf16
    matrix cores (the whole call runs under mlp.training_precision); a checkpoint resumes only at the precision it was written at."""
    settings = ckpt_mod.train_op_settings(lr, lr_decay, clip_norm, tf_epsilon, precision)
    ck = None
    if resume:
        ck, path = ckpt_mod.resume_state(checkpoint_dir, config, settings)
        log("resuming from %s (global step %d)" % (path, ck["global_step"]))
    start = ck["global_step"] if ck else 0
    n_steps = max(0, steps - start) if resume else steps
    torch.manual_seed(seed)
    data = KittiRpnBatches(dataset_dir, split, CLASSES, batch=batch, num_points=num_points, seed=seed, workers=workers,
                           state=ck["loader"] if ck else None)
    model, with_image = make_model(config, img_conv)
    if ck:
        model.load_state_dict(ck["model"], strict=True)
        ckpt_mod.load_drop_states(model, ck["drop_states"])
    parts = {}

    def loss_fn(m, inputs, geometry):
        seg_logits, head = m(inputs["xyz"], inputs["intensity"], geometry=geometry, img_fts=inputs.get("img_fts"),
                             calib=inputs.get("calib"))
        loss, p = m.loss(inputs["xyz"], seg_logits, head, inputs["label_cls"], inputs["label_reg"])
        parts.update(p)   # under a graph: the captured tensors, refreshed by every replay
        return loss

    def inputs_of(b):
        d = b.train_inputs()
        if not with_image:
            d.pop("img_fts"), d.pop("calib")
        return d

    try:
        steps_per_epoch = max(1, math.ceil(len(data.samples) / batch))
        cur = data.next()
        opt = MultiTensorAdam([p for p in model.parameters() if p.requires_grad], lr=lr, tf_epsilon=tf_epsilon, clip_norm=clip_norm,
                              lr_decay=lr_decay)
        if ck:
            opt.load_state_dict(ck["optimizer"])
        step = TrainStep(model, opt, inputs_of(cur), model.geometry(cur.xyz), graph=graph, loss_fn=loss_fn)
        if ck:
            ckpt_mod.load_rng_states(ck["rng"])          # after the capture: its warm-up draws were behind the saved run too
        keeper = ckpt_mod.Checkpointer(checkpoint_dir, checkpoint_every, max_checkpoints, config, settings, model, opt, data, start, log)
        prefetch = GeometryPrefetcher(model.geometry, depth=1)
        prefetch.submit(cur.xyz)
        losses = []
        t0 = time.perf_counter()
        for i in range(n_steps):
            g = start + i + 1                            # the global step this iteration completes
            nxt = data.next() if i + 1 < n_steps else None
            geo = prefetch.get()
            if nxt is not None:
                prefetch.submit(nxt.xyz)
            losses.append(step(geometry=geo, **inputs_of(cur)).clone())
            if log_every and (i + 1) % log_every == 0:
                if check_numerics:
                    keeper.check(losses, start + 1)
                log("step %d loss %.5f seg %.5f bin %.5f reg %.5f fg %d  lr %.3g  %.1f ms/step" % (
                    g, float(losses[-1]), float(parts["segmentation"]), float(parts["bin_classification"]),
                    float(parts["regression"]), int(parts["num_foreground"]), opt.lr_at(g - 1), 1e3 * (time.perf_counter() - t0) / (i + 1)))
            if keeper.due(g):
                keeper.write(g, nxt.position if nxt is not None else None, losses, start + 1)
            if (i + 1) % steps_per_epoch == 0:
                st = data.check_status()
                if st["empty"] or st["too_many_far"]:
                    log("status: %d frames with nothing in view, %d with more than P far points" % (st["empty"], st["too_many_far"]))
            cur = nxt
        st = data.check_status()
    finally:
        data.close()
    if check_numerics:
        keeper.check(losses, start + 1)
    if save:
        torch.save(model.state_dict(), save)
    out = [float(v) for v in torch.stack(losses).cpu()] if losses else []
    return out, st


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m heterofusionrcnn_amd.train_rpn",
                                 description="Train the RPN on KITTI frames (velodyne/, calib/, label_2/, image_2/ under DATASET_DIR).")
    ap.add_argument("dataset_dir")
    ap.add_argument("--split", default="train", help="a list file, or NAME for NAME.txt next to or inside DATASET_DIR")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--config", choices=CONFIGS, default="rpn_multiclass")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="path of the saved model state_dict (torch.save)")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8, help="host threads that read and decode the files")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--no-graph", action="store_true", help="eager steps instead of the captured hipGraph")
    ckpt_mod.add_train_op_arguments(ap, "rpn_multiclass.config")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    losses, st = train(args.dataset_dir, args.split, args.steps, args.batch, args.config, args.seed, args.save, args.log_every,
                       args.workers, graph=not args.no_graph, **ckpt_mod.train_op_kwargs(args))
    if losses:
        print("done: %d steps, first loss %.5f, last loss %.5f, status %s" % (len(losses), losses[0], losses[-1], st))
    else:
        print("done: no step left to run, status %s" % (st,))
    return 0


if __name__ == "__main__":
    sys.exit(main())
