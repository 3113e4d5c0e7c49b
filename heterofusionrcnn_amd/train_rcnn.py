"""Train the RCNN from KITTI files and the RPN's hand-off: python -m heterofusionrcnn_amd.train_rcnn DATASET_DIR HANDOFF_DIR
[--split train] [--steps N] [--batch 2] [--seed S] [--save rcnn.pt] [--no-graph]

HANDOFF_DIR is what export_rpn writes (proposals_and_scores/, rpn_feature/, proposals_iou/).  Batches come from
rcnn_data.KittiRcnnBatches (host reading one batch ahead, device split of the rows, flip and PCA jitter); the model is
rcnn_train.RcnnWithImageBranch (the RCNN with its own VGG pyramid, rcnn_multiclass.config), sized from the hand-off
(RcnnConfig(rpn_fts_channels=c, img_channels=...)); the step is graph_step.TrainStep with the device target layer, the fused
RCNN loss and optim.MultiTensorAdam, replayed from a captured hipGraph.  --save writes the RcnnTrainer's state_dict (weights,
image branch, the sampler's rng_state).

--reference-train-op (rcnn_multiclass.config:220-236), --checkpoint-dir / --checkpoint-every / --max-checkpoints and --resume as
in train_rpn (checkpoint.py).
"""
import argparse
import sys
import time

import torch

from . import checkpoint as ckpt_mod
from .graph_step import TrainStep
from .inference import ImgVggPyr
from .mlp import under_training_precision
from .optim import MultiTensorAdam
from .rcnn import RcnnConfig, RcnnModel
from .rcnn_data import KittiRcnnBatches
from .rcnn_train import RcnnTrainer, RcnnWithImageBranch


def make_trainer(rpn_fts_channels, img_conv=None, seed=0, path_drop=(0.9, 0.9)):
    """RcnnTrainer(RcnnWithImageBranch(RcnnModel, ImgVggPyr)) on the current device"""
    img_net = ImgVggPyr(img_conv) if img_conv else ImgVggPyr()
    cfg = RcnnConfig(rpn_fts_channels=rpn_fts_channels, img_channels=img_net.out_channel, path_drop=tuple(path_drop))
    return RcnnTrainer(RcnnWithImageBranch(RcnnModel(cfg), img_net), seed=seed).cuda().train()


CONFIG = "rcnn_multiclass"


@under_training_precision
def train(dataset_dir, handoff_dir, split="train", steps=100, batch=2, seed=0, save=None, log_every=10, workers=8, lr=1e-3,
          graph=True, img_conv=None, aug_list=None, log=print, clip_norm=0.0, lr_decay=None, tf_epsilon=False, check_numerics=False,
          checkpoint_dir=None, checkpoint_every=ckpt_mod.CHECKPOINT_INTERVAL, max_checkpoints=None, resume=False,
          precision="fp32"):
    """-> (list of the per-step losses of this run, read at the end; the trainer)

    The train-op, checkpoint, resume and precision keywords are train_rpn.train's (`steps` is the final global step when resuming)."""
    settings = ckpt_mod.train_op_settings(lr, lr_decay, clip_norm, tf_epsilon, precision)
    ck = None
    if resume:
        ck, path = ckpt_mod.resume_state(checkpoint_dir, CONFIG, settings)
        log("resuming from %s (global step %d)" % (path, ck["global_step"]))
    start = ck["global_step"] if ck else 0
    n_steps = max(0, steps - start) if resume else steps
    torch.manual_seed(seed)
    data = KittiRcnnBatches(dataset_dir, handoff_dir, split, mode="train", batch=batch, seed=seed, aug_list=aug_list, workers=workers,
                            state=ck["loader"] if ck else None)
    trainer = make_trainer(data.channels, img_conv, seed)
    if ck:
        trainer.load_state_dict(ck["model"], strict=True)
        ckpt_mod.load_drop_states(trainer, ck["drop_states"])
    parts = {}

    def loss_fn(m, inputs, geometry):
        loss, p = m(inputs["xyz"], inputs["rpn_fts"], inputs["intensity"], inputs["fg_mask"], inputs["proposals"],
                    inputs["proposal_count"], inputs["gt"], inputs["gt_count"], inputs["img_fts"], inputs["calib"])
        parts.update(p)   # under a graph: the captured tensors, refreshed by every replay
        return loss

    cur = data.next()
    opt = MultiTensorAdam([p for p in trainer.parameters() if p.requires_grad], lr=lr, tf_epsilon=tf_epsilon, clip_norm=clip_norm,
                          lr_decay=lr_decay)
    if ck:
        opt.load_state_dict(ck["optimizer"])
    step = TrainStep(trainer, opt, cur.train_inputs(), None, graph=graph, loss_fn=loss_fn)
    if ck:
        ckpt_mod.load_rng_states(ck["rng"])          # after the capture: its warm-up draws were behind the saved run too
    keeper = ckpt_mod.Checkpointer(checkpoint_dir, checkpoint_every, max_checkpoints, CONFIG, settings, trainer, opt, data, start, log)
    losses = []
    t0 = time.perf_counter()
    try:
        for i in range(n_steps):
            g = start + i + 1                        # the global step this iteration completes
            nxt = data.next() if i + 1 < n_steps else None
            losses.append(step(**cur.train_inputs()).clone())
            if log_every and (i + 1) % log_every == 0:
                if check_numerics:
                    keeper.check(losses, start + 1)
                st = parts["stats"].sum(dim=0).tolist()
                log("step %d loss %.5f cls %.5f bin %.5f reg %.5f fg %d bg %d  lr %.3g  %.1f ms/step" % (
                    g, float(losses[-1]), float(parts["box_classification"]), float(parts["bin_classification"]),
                    float(parts["regression"]), st[2], st[3], opt.lr_at(g - 1), 1e3 * (time.perf_counter() - t0) / (i + 1)))
            if keeper.due(g):
                keeper.write(g, nxt.position if nxt is not None else None, losses, start + 1)
            cur = nxt
        status = data.check_status()
        if check_numerics:
            keeper.check(losses, start + 1)
    finally:
        data.close()
    if status["bad_fg"]:
        log("status: %d frames whose fg column held a value other than 0 / 1" % status["bad_fg"])
    if save:
        torch.save(trainer.state_dict(), save)
    out = [float(v) for v in torch.stack(losses).cpu()] if losses else []
    return out, trainer


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m heterofusionrcnn_amd.train_rcnn",
                                 description="Train the RCNN (with its VGG image branch) on KITTI frames (calib/, label_2/, image_2/ "
                                             "under DATASET_DIR) and the RPN hand-off that export_rpn wrote to HANDOFF_DIR.")
    ap.add_argument("dataset_dir")
    ap.add_argument("handoff_dir")
    ap.add_argument("--split", default="train", help="a list file, or NAME for NAME.txt next to or inside DATASET_DIR")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=2, help="frames per step (rcnn_multiclass.config:218)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="path of the saved trainer state_dict (torch.save)")
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8, help="host threads that read and decode the files")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--no-graph", action="store_true", help="eager steps instead of the captured hipGraph")
    ckpt_mod.add_train_op_arguments(ap, "rcnn_multiclass.config")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    losses, _ = train(args.dataset_dir, args.handoff_dir, args.split, args.steps, args.batch, args.seed, args.save, args.log_every,
                      args.workers, graph=not args.no_graph, **ckpt_mod.train_op_kwargs(args))
    if losses:
        print("done: %d steps, first loss %.5f, last loss %.5f" % (len(losses), losses[0], losses[-1]))
    else:
        print("done: no step left to run")
    return 0


if __name__ == "__main__":
    sys.exit(main())
