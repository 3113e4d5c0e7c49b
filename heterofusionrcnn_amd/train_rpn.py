"""Train the RPN from KITTI files: python -m heterofusionrcnn_amd.train_rpn DATASET_DIR [--split train] [--steps N] ...

The run is train_loop.run over RpnStage: batches from kitti_data.KittiRpnBatches (device batch assembly, one batch ahead), the step
graph_step.TrainStep (replayed from a captured hipGraph), the geometry of the next batch prefetched on a side stream.  Configs that
fuse the image train RpnWithImageBranch(model, ImgVggPyr()), the reference's whole step.  --save writes the model's state_dict.

--reference-train-op runs the reference's train op (rpn_multiclass.config:204-224 train_config, hf/core/trainer.py:68-84):
Adam with TensorFlow's epsilon, per-tensor gradient clipping at 1.0 and a staircase exponential decay (0.001 x world, 20 000
steps, factor 0.8); a NaN / Inf loss then stops the run (check_numerics).  --checkpoint-dir writes a checkpoint (model,
optimizer, global step, dropout counters, generator states, loader position: checkpoint.py) every --checkpoint-every steps,
and --resume continues from the newest one up to the global step --steps.
"""
import argparse
import math
import sys

from . import checkpoint as ckpt_mod
from . import image_pyramid
from . import rpn as rpn_mod
from . import train_loop
from .determinism import IMAGE_CONFIGS_REFUSED, as_level, level, refuse_image_config
from .graph_step import rpn_loss_parts
from .inference import CLASSES, ImgVggPyr
from .kitti_data import KittiRpnBatches
from .mlp import under_training_precision

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


class RpnStage:
    """what train_loop.run asks of a stage, for the RPN configs"""
    loss = staticmethod(rpn_loss_parts)

    def __init__(self, config, img_conv, **loader):
        self.config, self.img_conv, self.loader = config, img_conv, loader

    def open(self, state):
        return KittiRpnBatches(state=state, **self.loader)

    def build(self, data):
        self.steps_per_epoch = max(1, math.ceil(len(data.samples) / self.loader["batch"]))
        model, self.with_image = make_model(self.config, self.img_conv)
        self.geometry = model.geometry                   # of the coordinates alone: prefetched one batch ahead
        return model

    def inputs(self, b):
        d = b.train_inputs()
        if not self.with_image:
            d.pop("img_fts"), d.pop("calib")
        return d

    def log_parts(self, parts):
        return "seg %.5f bin %.5f reg %.5f fg %d" % (float(parts["segmentation"]), float(parts["bin_classification"]),
                                                     float(parts["regression"]), int(parts["num_foreground"]))

    def epoch_status(self, i, data, log):
        if (i + 1) % self.steps_per_epoch == 0:
            st = data.check_status()
            if st["empty"] or st["too_many_far"]:
                log("status: %d frames with nothing in view, %d with more than P far points" % (st["empty"], st["too_many_far"]))

    def finish(self, status, log):
        return status


@under_training_precision
def train(dataset_dir, split="train", steps=100, batch=8, config="rpn_multiclass", seed=0, save=None, log_every=10, workers=8,
          lr=1e-3, graph=True, img_conv=None, num_points=16384, log=print, clip_norm=0.0, lr_decay=None, tf_epsilon=False,
          check_numerics=False, checkpoint_dir=None, checkpoint_every=ckpt_mod.CHECKPOINT_INTERVAL, max_checkpoints=None, resume=False,
          precision="fp32", image_train_branch="torch", deterministic=False):
    """-> (list of the per-step losses of this run, floats read at the end; the loader status)
    clip_norm / lr_decay / tf_epsilon: optim.MultiTensorAdam's (ckpt_mod.reference_train_op() holds the reference's values);
    check_numerics: a NaN / Inf loss raises FloatingPointError at the next log point (always before a checkpoint is written);
    checkpoint_dir: a checkpoint every checkpoint_every global steps, the newest max_checkpoints kept; resume: continue from the
    newest checkpoint there, `steps` then being the final global step.  precision "bf16": the wide dense layers train on the bf16
    matrix cores (the whole call runs under mlp.training_precision); a checkpoint resumes only at the precision it was written at.
    image_train_branch: "native" trains the image pyramid on this package's kernels (image_pyramid.train_branch; no atomics, allowed at
    every deterministic level); "torch" is the stock module on the vendor library.
    deterministic: True or "image", the run is inside determinism.deterministic at that level (bit-reproducible: train_loop.run).  True
    trains rpn_multiclass_points only: the config that fuses the image is refused before anything is built.  "image" trains every
    config, the image-feature gradients in their ordered form."""
    if (as_level(deterministic) or level()) is True and config == "rpn_multiclass":
        refuse_image_config("train_rpn, config rpn_multiclass")
    stage = RpnStage(config, img_conv, dataset_dir=dataset_dir, split=split, classes=CLASSES, batch=batch, num_points=num_points,
                     seed=seed, workers=workers)
    # the scope holds for the whole run: the capture of the step and every eager step read it where ImgVggPyr.forward runs
    with image_pyramid.train_branch(image_train_branch):
        return train_loop.run(stage, steps, seed, save, log_every, lr, graph, log, clip_norm, lr_decay, tf_epsilon, check_numerics,
                              checkpoint_dir, checkpoint_every, max_checkpoints, resume, precision,
                              deterministic=deterministic)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m heterofusionrcnn_amd.train_rpn",
                                 description="Train the RPN on KITTI frames (velodyne/, calib/, label_2/, image_2/ under DATASET_DIR).")
    ckpt_mod.add_run_arguments(ap, "model")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--config", choices=CONFIGS, default="rpn_multiclass")
    ckpt_mod.add_train_op_arguments(ap, "rpn_multiclass.config")
    ap.add_argument("--image-train-branch", choices=image_pyramid.TRAIN_BRANCHES, default="torch",
                    help="the image pyramid's forward and backward: torch (the vendor library) or native (this package's NHWC "
                         "fp32-MFMA kernels, no atomics; allowed at every --deterministic level)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.deterministic and not args.deterministic_image and args.config == "rpn_multiclass":
        ap.error("--deterministic with --config rpn_multiclass: " + IMAGE_CONFIGS_REFUSED)
    losses, st = train(args.dataset_dir, args.split, args.steps, args.batch, args.config, args.seed, args.save, args.log_every,
                       args.workers, graph=not args.no_graph, deterministic=ckpt_mod.deterministic_level(args), image_train_branch=args.image_train_branch,
                       **ckpt_mod.train_op_kwargs(args))
    if losses:
        print("done: %d steps, first loss %.5f, last loss %.5f, status %s" % (len(losses), losses[0], losses[-1], st))
    else:
        print("done: no step left to run, status %s" % (st,))
    return 0


if __name__ == "__main__":
    sys.exit(main())
