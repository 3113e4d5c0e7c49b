"""Train the RCNN from KITTI files and the RPN's hand-off: python -m heterofusionrcnn_amd.train_rcnn DATASET_DIR HANDOFF_DIR
[--split train] [--steps N] [--batch 2] [--seed S] [--save rcnn.pt] [--no-graph]

HANDOFF_DIR is what export_rpn writes (proposals_and_scores/, rpn_feature/, proposals_iou/).  The run is train_loop.run over
RcnnStage: batches from rcnn_data.KittiRcnnBatches (host reading one batch ahead, device split of the rows, flip and PCA jitter);
the model rcnn_train.RcnnWithImageBranch (the RCNN with its own VGG pyramid, rcnn_multiclass.config), sized from the hand-off
(RcnnConfig(rpn_fts_channels=c, img_channels=...)); the step graph_step.TrainStep with the device target layer, the fused RCNN loss
and optim.MultiTensorAdam, replayed from a captured hipGraph.  --save writes the RcnnTrainer's state_dict (weights, image branch,
the sampler's rng_state).  --reference-train-op (rcnn_multiclass.config:220-236), --checkpoint-dir / --checkpoint-every /
--max-checkpoints and --resume as in train_rpn (checkpoint.py).
"""
import argparse
import sys

from . import checkpoint as ckpt_mod
from . import image_pyramid
from . import train_loop
from .determinism import IMAGE_CONFIGS_REFUSED, as_level, level, refuse_image_config
from .inference import ImgVggPyr
from .mlp import under_training_precision
from .rcnn import RcnnConfig, RcnnModel
from .rcnn_data import KittiRcnnBatches
from .rcnn_train import RcnnTrainer, RcnnWithImageBranch, rcnn_train_loss_parts

CONFIG = "rcnn_multiclass"

def make_trainer(rpn_fts_channels, img_conv=None, seed=0, path_drop=(0.9, 0.9)):
    """RcnnTrainer(RcnnWithImageBranch(RcnnModel, ImgVggPyr)) on the current device"""
    img_net = ImgVggPyr(img_conv) if img_conv else ImgVggPyr()
    cfg = RcnnConfig(rpn_fts_channels=rpn_fts_channels, img_channels=img_net.out_channel, path_drop=tuple(path_drop))
    return RcnnTrainer(RcnnWithImageBranch(RcnnModel(cfg), img_net), seed=seed).cuda().train()


class RcnnStage:
    """what train_loop.run asks of a stage, for the RCNN: no geometry outside the step, nothing at the end of an epoch"""
    config, geometry, epoch_status = CONFIG, None, None
    loss = staticmethod(rcnn_train_loss_parts)

    def __init__(self, img_conv, **loader):
        self.img_conv, self.loader = img_conv, loader

    def open(self, state):
        return KittiRcnnBatches(mode="train", state=state, **self.loader)

    def build(self, data):
        self.trainer = make_trainer(data.channels, self.img_conv, self.loader["seed"])
        return self.trainer

    def inputs(self, b):
        return b.train_inputs()

    def log_parts(self, parts):
        st = parts["stats"].sum(dim=0).tolist()
        return "cls %.5f bin %.5f reg %.5f fg %d bg %d" % (float(parts["box_classification"]), float(parts["bin_classification"]),
                                                           float(parts["regression"]), st[2], st[3])

    def finish(self, status, log):
        if status["bad_fg"]:
            log("status: %d frames whose fg column held a value other than 0 / 1" % status["bad_fg"])
        return self.trainer


@under_training_precision
def train(dataset_dir, handoff_dir, split="train", steps=100, batch=2, seed=0, save=None, log_every=10, workers=8, lr=1e-3,
          graph=True, img_conv=None, aug_list=None, log=print, clip_norm=0.0, lr_decay=None, tf_epsilon=False, check_numerics=False,
          checkpoint_dir=None, checkpoint_every=ckpt_mod.CHECKPOINT_INTERVAL, max_checkpoints=None, resume=False,
          precision="fp32", image_train_branch="torch", deterministic=False):
    """-> (list of the per-step losses of this run, read at the end; the trainer)
    The train-op, checkpoint, resume, precision, image_train_branch and deterministic keywords are train_rpn.train's (`steps` is the final global step when resuming);
    the RCNN fuses the image, so deterministic=True is refused before anything is built and deterministic="image" is the level it trains at."""
    if (as_level(deterministic) or level()) is True:
        refuse_image_config("train_rcnn")
    stage = RcnnStage(img_conv, dataset_dir=dataset_dir, handoff_dir=handoff_dir, split=split, batch=batch, seed=seed, aug_list=aug_list,
                      workers=workers)
    # the scope holds for the whole run: the capture of the step and every eager step read it where ImgVggPyr.forward runs
    with image_pyramid.train_branch(image_train_branch):
        return train_loop.run(stage, steps, seed, save, log_every, lr, graph, log, clip_norm, lr_decay, tf_epsilon, check_numerics,
                              checkpoint_dir, checkpoint_every, max_checkpoints, resume, precision,
                              deterministic=deterministic)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m heterofusionrcnn_amd.train_rcnn",
                                 description="Train the RCNN (with its VGG image branch) on KITTI frames (calib/, label_2/, image_2/ "
                                             "under DATASET_DIR) and the RPN hand-off that export_rpn wrote to HANDOFF_DIR.")
    ckpt_mod.add_run_arguments(ap, "trainer")
    ap.add_argument("handoff_dir")
    ap.add_argument("--batch", type=int, default=2, help="frames per step (rcnn_multiclass.config:218)")
    ckpt_mod.add_train_op_arguments(ap, "rcnn_multiclass.config")
    ap.add_argument("--image-train-branch", choices=image_pyramid.TRAIN_BRANCHES, default="torch",
                    help="the image pyramid's forward and backward: torch (the vendor library) or native (this package's NHWC "
                         "fp32-MFMA kernels, no atomics; allowed at every --deterministic level)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.deterministic and not args.deterministic_image:
        ap.error("--deterministic: " + IMAGE_CONFIGS_REFUSED)
    losses, _ = train(args.dataset_dir, args.handoff_dir, args.split, args.steps, args.batch, args.seed, args.save, args.log_every,
                      args.workers, graph=not args.no_graph, deterministic=ckpt_mod.deterministic_level(args), image_train_branch=args.image_train_branch,
                       **ckpt_mod.train_op_kwargs(args))
    if losses:
        print("done: %d steps, first loss %.5f, last loss %.5f" % (len(losses), losses[0], losses[-1]))
    else:
        print("done: no step left to run")
    return 0


if __name__ == "__main__":
    sys.exit(main())
