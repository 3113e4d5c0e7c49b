"""The one training loop of train_rpn and train_rcnn: run(stage, ...) puts a resumable run together, iterates and reads back.
The order is the policy (tests/test_train_loop_cpu.py, tests/test_train_resume.py): resume check, seed, loader, module, checkpoint
weights and dropout counters, first batch, optimizer, optimizer state, capture, generator states last; a checkpoint records the
position of the first batch the run has not trained on; the loader, once open, is closed on every way out.

A stage (train_rpn.RpnStage, train_rcnn.RcnnStage) is what differs: `config` (the checkpoint's config name), open(state) -> loader,
build(data) -> module, inputs(batch) -> TrainStep's dict, `geometry` (coordinates -> geometry, known after build; None: the step takes
none), loss(module, inputs, geometry) -> (loss, parts), log_parts(parts) -> the middle of the log line, `epoch_status` (None, or
(i, data, log) called at the end of iteration i) and finish(final loader status, log) -> the second value run returns.
"""
import time

import torch

from . import checkpoint as ckpt_mod
from .determinism import as_level, deterministic as deterministic_mode, level
from .graph_step import TrainStep
from .optim import MultiTensorAdam
from .pipeline import GeometryPrefetcher


def run(stage, steps, seed, save, log_every, lr, graph, log, clip_norm, lr_decay, tf_epsilon, check_numerics, checkpoint_dir,
        checkpoint_every, max_checkpoints, resume, precision, deterministic=False):
    """-> (list of the per-step losses of this run, floats read at the end; stage.finish(the loader's final status, log))

    The arguments are train_rpn.train's, which documents them; the caller runs under mlp.training_precision(precision).  deterministic: the
    whole run -- the capture and every step -- is inside determinism.deterministic(deterministic), True or "image": no route whose sum has
    no fixed order runs; two runs from one state then give the same bits ("Reproducible training")."""
    with deterministic_mode(as_level(deterministic) or level()):       # the level as asked for; a caller's own scope stays on
        return _run(stage, steps, seed, save, log_every, lr, graph, log, clip_norm, lr_decay, tf_epsilon, check_numerics, checkpoint_dir,
                    checkpoint_every, max_checkpoints, resume, precision)


def _run(stage, steps, seed, save, log_every, lr, graph, log, clip_norm, lr_decay, tf_epsilon, check_numerics, checkpoint_dir,
         checkpoint_every, max_checkpoints, resume, precision):
    settings = ckpt_mod.train_op_settings(lr, lr_decay, clip_norm, tf_epsilon, precision)
    ck = None
    if resume:
        ck, path = ckpt_mod.resume_state(checkpoint_dir, stage.config, settings)
        log("resuming from %s (global step %d)" % (path, ck["global_step"]))
    start = ck["global_step"] if ck else 0
    n_steps = max(0, steps - start) if resume else steps
    torch.manual_seed(seed)
    data = stage.open(ck["loader"] if ck else None)
    try:
        module = stage.build(data)
        if ck:
            module.load_state_dict(ck["model"], strict=True)
            ckpt_mod.load_drop_states(module, ck["drop_states"])
        parts = {}

        def loss_fn(m, inputs, geometry):
            loss, p = stage.loss(m, inputs, geometry)
            parts.update(p)   # under a graph: the captured tensors, refreshed by every replay
            return loss

        cur = data.next()
        opt = MultiTensorAdam([p for p in module.parameters() if p.requires_grad], lr=lr, tf_epsilon=tf_epsilon, clip_norm=clip_norm,
                              lr_decay=lr_decay)
        if ck:
            opt.load_state_dict(ck["optimizer"])
        step = TrainStep(module, opt, stage.inputs(cur), stage.geometry(cur.xyz) if stage.geometry else None, graph=graph,
                         loss_fn=loss_fn)
        if ck:
            ckpt_mod.load_rng_states(ck["rng"])          # after the capture: its warm-up draws were behind the saved run too
        keeper = ckpt_mod.Checkpointer(checkpoint_dir, checkpoint_every, max_checkpoints, stage.config, settings, module, opt, data, start, log)
        prefetch = GeometryPrefetcher(stage.geometry, depth=1) if stage.geometry else None
        if prefetch is not None:
            prefetch.submit(cur.xyz)
        losses, geo = [], None
        t0 = time.perf_counter()
        for i in range(n_steps):
            g = start + i + 1                            # the global step this iteration completes
            nxt = data.next() if i + 1 < n_steps else None
            if prefetch is not None:                     # (it has a length: empty is false)
                geo = prefetch.get()
                if nxt is not None:
                    prefetch.submit(nxt.xyz)
            losses.append(step(geometry=geo, **stage.inputs(cur)).clone())
            if log_every and (i + 1) % log_every == 0:
                if check_numerics:
                    keeper.check(losses, start + 1)
                log("step %d loss %.5f %s  lr %.3g  %.1f ms/step" % (
                    g, float(losses[-1]), stage.log_parts(parts), opt.lr_at(g - 1), 1e3 * (time.perf_counter() - t0) / (i + 1)))
            if keeper.due(g):
                keeper.write(g, nxt.position if nxt is not None else None, losses, start + 1)
            if stage.epoch_status:
                stage.epoch_status(i, data, log)
            cur = nxt
        status = data.check_status()
    finally:
        data.close()
    if check_numerics:
        keeper.check(losses, start + 1)
    result = stage.finish(status, log)
    if save:
        torch.save(module.state_dict(), save)
    return [float(v) for v in torch.stack(losses).cpu()] if losses else [], result
