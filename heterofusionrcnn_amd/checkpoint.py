"""Training checkpoints shared by train_rpn and train_rcnn (hf/core/trainer.py:131-176: a checkpoint every checkpoint_interval
steps, the newest restored at start-up with the Adam slots and the global step).

One file per checkpoint, <dir>/ckpt-%08d.pt named by the global step (the reference's -{:08d} suffix).  A file is written under a
temporary name in the same directory and moved into place with os.replace, so an interrupted run never leaves a truncated
newest checkpoint; only the newest `keep` files stay.  A checkpoint is one torch.save'd dict:

  model          the model's (or RcnnTrainer's) state_dict, the keys --save writes
  optimizer      optim.MultiTensorAdam.state_dict()
  global_step    steps done
  drop_states    {module name: BatchNormReLU.drop_state} (both words: base seed and call count; the buffer itself stays out of
                 the state_dict, so --save files and export_rpn's strict load keep their keys)
  rng            {"cuda": the device generator's state (path drop), "cpu": torch's CPU generator state}
  loader         the position of the first batch the run had not trained on (kitti_data.KittiRpnBatches / rcnn_data
                 .KittiRcnnBatches state_dict format)
  config         the config name; settings: the train-op settings (resume refuses another config or other settings)
"""
import os
import re

import torch

PATTERN = "ckpt-%08d.pt"
_NAME = re.compile(r"^ckpt-(\d{8,})\.pt$")


def checkpoint_path(directory, global_step):
    return os.path.join(directory, PATTERN % int(global_step))


def list_checkpoints(directory):
    """[(global_step, path)] of the complete checkpoint files in `directory`, oldest first (temporary files are not listed)"""
    if not os.path.isdir(directory):
        return []
    out = []
    for name in os.listdir(directory):
        m = _NAME.match(name)
        if m:
            out.append((int(m.group(1)), os.path.join(directory, name)))
    return sorted(out)


def latest_checkpoint(directory):
    """the path of the newest checkpoint in `directory`, or None"""
    found = list_checkpoints(directory)
    return found[-1][1] if found else None


def save_checkpoint(directory, global_step, payload, keep=None):
    """write `payload` (a dict; global_step is added) as <directory>/ckpt-%08d.pt through a temporary file and os.replace, then
    delete all but the newest `keep` checkpoints (None: keep all) -> the path"""
    if keep is not None and int(keep) < 1:
        raise ValueError("keep must be >= 1 (or None), got %r" % (keep,))
    os.makedirs(directory, exist_ok=True)
    path = checkpoint_path(directory, global_step)
    tmp = os.path.join(directory, ".%s.tmp-%d" % (os.path.basename(path), os.getpid()))
    data = dict(payload)
    data["global_step"] = int(global_step)
    try:
        with open(tmp, "wb") as f:
            torch.save(data, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    if keep is not None:
        for _, old in list_checkpoints(directory)[:-int(keep)]:
            os.remove(old)
    return path


def load_checkpoint(path):
    """the dict save_checkpoint wrote, tensors on the CPU"""
    return torch.load(path, map_location="cpu", weights_only=True)


def is_checkpoint(obj):
    return isinstance(obj, dict) and "model" in obj and "optimizer" in obj and "global_step" in obj


def model_state(obj):
    """a model state_dict from either a --save file's content or a checkpoint's"""
    return obj["model"] if is_checkpoint(obj) else obj


# ---------------------------------------------------------------------------------------------- the trainers' train op
CHECKPOINT_INTERVAL = 2000          # the train_config checkpoint_interval of rpn_multiclass.config and rcnn_multiclass.config


def reference_train_op(world=1):
    """the train_config of rpn_multiclass.config:204-224 and rcnn_multiclass.config:220-236 (the same values) as train()
    keywords: lr 0.001 x world (hf/core/trainer.py scales the initial learning rate by hvd.size()), staircase decay every 20 000
    steps by 0.8, clip_gradient_norm 1.0, tf.train.AdamOptimizer, check_numerics on the total loss"""
    return {"lr": 0.001 * world, "lr_decay": (20000, 0.8, True), "clip_norm": 1.0, "tf_epsilon": True, "check_numerics": True}


def train_op_settings(lr, lr_decay, clip_norm, tf_epsilon, precision="fp32"):
    """what a checkpoint records of the train op (resume refuses other values).  "precision" is recorded only when it is not fp32:
    fp32 checkpoints keep their format, and a checkpoint resumes only at the precision it was written at"""
    settings = {"lr": float(lr), "lr_decay": None if lr_decay is None else tuple(lr_decay), "clip_norm": float(clip_norm),
                "tf_epsilon": bool(tf_epsilon)}
    if precision != "fp32":
        settings["precision"] = str(precision)
    return settings


class Checkpointer:
    """the checkpoint side of a training loop: the non-finite check on the losses since the last check (one synchronising read,
    at log points and before a checkpoint) and the writes"""

    def __init__(self, directory, every, keep, config, settings, module, opt, data, start_step, log):
        self.directory, self.every, self.keep = directory, int(every), keep
        self.config, self.settings, self.module, self.opt, self.data, self.log = config, settings, module, opt, data, log
        self.checked = start_step          # global steps whose loss is known to be finite

    def check(self, losses, first_step):
        """losses[k] is global step first_step + k; FloatingPointError at the first NaN / Inf loss not yet checked"""
        todo = losses[self.checked - first_step + 1:]
        bad = first_nonfinite(todo, self.checked + 1)
        if bad is not None:
            raise FloatingPointError("non-finite loss %r at global step %d" % (float(losses[bad - first_step]), bad))
        self.checked += len(todo)

    def due(self, global_step):
        return bool(self.directory) and self.every > 0 and global_step % self.every == 0

    def write(self, global_step, position, losses, first_step):
        self.check(losses, first_step)
        path = save_checkpoint(self.directory, global_step, {
            "model": self.module.state_dict(), "optimizer": self.opt.state_dict(), "drop_states": drop_states(self.module),
            "rng": rng_states(), "loader": self.data.state_dict(position), "config": self.config,
            "settings": self.settings}, keep=self.keep)
        self.log("checkpoint %s" % path)
        return path


def resume_state(checkpoint_dir, config, settings):
    """the newest checkpoint under checkpoint_dir, checked against this run's config and settings"""
    if not checkpoint_dir:
        raise ValueError("resume needs a checkpoint directory")
    path = latest_checkpoint(checkpoint_dir)
    if path is None:
        raise FileNotFoundError("no checkpoint (ckpt-NNNNNNNN.pt) in %s" % checkpoint_dir)
    ck = load_checkpoint(path)
    check_resumable(ck, config, settings, path)
    return ck, path


def add_run_arguments(ap, saved):
    """DATASET_DIR and the flags of a run that train_rpn and train_rcnn share (`saved`: what --save holds, "model" / "trainer")"""
    ap.add_argument("dataset_dir")
    ap.add_argument("--split", default="train", help="a list file, or NAME for NAME.txt next to or inside DATASET_DIR")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save", default=None, help="path of the saved %s state_dict (torch.save)" % saved)
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--workers", type=int, default=8, help="host threads that read and decode the files")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--no-graph", action="store_true", help="eager steps instead of the captured hipGraph")
    ap.add_argument("--deterministic", action="store_true",
                    help="bit-reproducible training: every route whose sum has no fixed order is refused; the configurations that fuse the "
                         "image (train_rcnn, train_rpn --config rpn_multiclass) do not run under it")
    ap.add_argument("--deterministic-image", action="store_true",
                    help="bit-reproducible training of every configuration: --deterministic, and the image-feature gradients (project_gather, "
                         "image_crop_and_resize) summed in a fixed order instead of by fp32 atomics")


def add_train_op_arguments(ap, config_file):
    """--reference-train-op and the checkpoint flags (train_rpn and train_rcnn)"""
    ap.add_argument("--reference-train-op", action="store_true",
                    help="the train op of %s: lr 0.001 x world, staircase decay by 0.8 every 20000 steps, per-tensor gradient "
                         "clipping at 1.0, TensorFlow's Adam epsilon, stop on a NaN / Inf loss (overrides --lr)" % config_file)
    ap.add_argument("--checkpoint-dir", default=None, help="write checkpoints (ckpt-%%08d.pt by global step) into this directory")
    ap.add_argument("--checkpoint-every", type=int, default=CHECKPOINT_INTERVAL,
                    help="global steps between checkpoints (default %d, the configs' checkpoint_interval)" % CHECKPOINT_INTERVAL)
    ap.add_argument("--max-checkpoints", type=int, default=None, help="keep only the newest K checkpoints")
    ap.add_argument("--resume", action="store_true",
                    help="continue from the newest checkpoint in --checkpoint-dir; --steps is then the final global step")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32",
                    help="bf16: the wide dense layers train on the bf16 matrix cores (fp32 accumulation, tensors, master weights and "
                         "Adam; a checkpoint resumes only at the precision it was written at)")


def deterministic_level(args):
    """the `deterministic` keyword of train() from the parsed flags: False, True, or "image" (--deterministic-image implies the mode)"""
    return "image" if args.deterministic_image else bool(args.deterministic)


def train_op_kwargs(args, world=1):
    """the train() keywords of the parsed train-op and checkpoint flags"""
    if args.max_checkpoints is not None and args.max_checkpoints < 1:
        raise SystemExit("--max-checkpoints must be >= 1")
    if args.resume and not args.checkpoint_dir:
        raise SystemExit("--resume needs --checkpoint-dir")
    kw = reference_train_op(world) if args.reference_train_op else {"lr": args.lr}
    kw.update(checkpoint_dir=args.checkpoint_dir, checkpoint_every=args.checkpoint_every, max_checkpoints=args.max_checkpoints,
              resume=args.resume, precision=args.precision)
    return kw


# ---------------------------------------------------------------------------------------------- pieces of the run's state
def drop_states(module):
    """{module name: drop_state (2,) int64 on the CPU} of every fused-dropout BatchNormReLU under `module`"""
    return {name: m.drop_state.detach().cpu().clone() for name, m in module.named_modules()
            if isinstance(getattr(m, "drop_state", None), torch.Tensor)}


def load_drop_states(module, states):
    """copy saved drop_state pairs back in place; ValueError when the modules differ"""
    mods = {name: m for name, m in module.named_modules() if isinstance(getattr(m, "drop_state", None), torch.Tensor)}
    if set(mods) != set(states):
        raise ValueError("checkpoint: the dropout layers differ (%d saved, %d in the model)" % (len(states), len(mods)))
    with torch.no_grad():
        for name, m in mods.items():
            m.drop_state.copy_(states[name])


def rng_states():
    return {"cuda": torch.cuda.get_rng_state(), "cpu": torch.get_rng_state()}


def load_rng_states(states):
    torch.cuda.set_rng_state(states["cuda"])
    torch.set_rng_state(states["cpu"])


def check_resumable(ckpt, config, settings, path):
    """ValueError unless the checkpoint was written by the same config with the same train-op settings"""
    if ckpt.get("config") != config:
        raise ValueError("%s was written by config %r, this run is %r" % (path, ckpt.get("config"), config))
    if ckpt.get("settings") != settings:
        raise ValueError("%s was written with train-op settings %r, this run has %r" % (path, ckpt.get("settings"), settings))


def first_nonfinite(losses, first_step):
    """losses: device scalars of consecutive steps, the first one global step `first_step` -> the global step of the first NaN /
    Inf loss, or None (one synchronising read)"""
    if not losses:
        return None
    bad = (~torch.isfinite(torch.stack(losses))).nonzero()
    return None if bad.numel() == 0 else first_step + int(bad[0, 0])
