"""Adam for the train step: every parameter tensor in ONE launch (csrc/optim.hip, hf_adam_multi).

The reference's step ends in tf.train.AdamOptimizer.apply_gradients (hf/builders/optimizer_builder.py:59-64, wrapped by
hvd.DistributedOptimizer in hf/core/trainer.py:71).  torch.optim.Adam(fused=True) needs seven launches for this model's 260
tensors (the tensor list travels in kernel arguments) and moves 1.2 TB/s; here the list is a table in device memory and a
workgroup looks its chunk up.  The gradients are read where autograd left them: when their addresses change (eager steps
allocate fresh gradients; a captured graph does not) the table is rewritten and uploaded, otherwise a step is two launches
(the step counter, the update).

Who owns which table.  Eager steps and captured steps may be mixed freely on one optimizer (graph_step.TrainStep does: its
warm-up steps and its capture share one), so they never share a table:
  eager steps   launch on ONE device table / chunk map / chunk count that only eager uploads write.  The cache key `_key` is the
                gradient addresses of the last EAGER upload, which is exactly what that table holds: no capture and no replay
                touches either.  An eager step uploads iff its gradients' addresses (or the set of tensors that have one)
                differ from the key; eager steps on unmoved gradients upload once.
  a capture     takes a device table, a chunk map and pinned staging of its own for good and ALWAYS records its own upload
                nodes and its own chunk count, whatever the key says: every replay rewrites and reads only that table, and no
                later eager step can change what a replay updates.  It neither reads nor sets the key.
`table_uploads` counts the uploads Python issued (eager uploads, and one per capture while it is recorded); a replay issues none.

`tf_epsilon=True` (default) is TensorFlow's update  p -= lr sqrt(1-b2^t)/(1-b1^t) m / (sqrt(v) + eps); False is
torch.optim.Adam's placement of epsilon (tests/test_optim.py pins the arithmetic of that mode to torch's own optimizer).

The reference's train op (slim.learning.create_train_op(..., clip_gradient_norm=1.0), hf/core/trainer.py:77-84, with
tf.train.exponential_decay, hf/builders/optimizer_builder.py:102-110) is opt-in: `clip_norm > 0` clips every tensor's averaged
gradient to that L2 norm (one more launch per step: the per-chunk sums of squares, hf_adam_sqnorm_partials), `lr_decay=(decay_steps,
decay_factor[, staircase=True])` decays the learning rate from the device step counter, so a captured step follows the schedule at
every replay.  With both off a step is the launch above, unchanged.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr


class _Entry(ctypes.Structure):
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("numel", ctypes.c_longlong)]


def _check_decay(lr_decay):
    """(decay_steps, decay_factor[, staircase]) -> (float, float, bool), or None"""
    if lr_decay is None:
        return None
    if not 2 <= len(lr_decay) <= 3:
        raise ValueError("lr_decay must be (decay_steps, decay_factor[, staircase])")
    steps, factor = float(lr_decay[0]), float(lr_decay[1])
    staircase = bool(lr_decay[2]) if len(lr_decay) == 3 else True
    if not (steps > 0 and factor > 0):
        raise ValueError("lr_decay: decay_steps and decay_factor must be > 0, got %r" % (tuple(lr_decay),))
    return steps, factor, staircase


def lr_at(lr, lr_decay, global_step):
    """tf.train.exponential_decay(lr, global_step, decay_steps, decay_factor, staircase) in fp32, as the update computes it (Adam
    step t runs at global step t - 1); lr_decay None: lr"""
    lr_decay = _check_decay(lr_decay)
    lr = np.float32(lr)
    if lr_decay is None:
        return float(lr)
    q = np.float32(global_step) / np.float32(lr_decay[0])
    if lr_decay[2]:
        q = np.floor(q)
    return float(lr * np.power(np.float32(lr_decay[1]), q, dtype=np.float32))


class MultiTensorAdam:
    """step() semantics of torch.optim.Adam(params, lr, betas, eps) without weight decay / amsgrad.  Parameters whose .grad is
    None at a step are skipped for that step (their moments stay), as the framework optimizers do.

    clip_norm > 0: per-tensor tf.clip_by_norm of the averaged gradient before the update.  lr_decay: (decay_steps, decay_factor,
    staircase=True) for tf.train.exponential_decay of lr.  state_dict() / load_state_dict(): the moments, the step counter (the
    global step), the hyper-parameters and a fingerprint of the parameter list (count and shapes)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, tf_epsilon=True, grad_scale=1.0, clip_norm=0.0, lr_decay=None):
        if not float(clip_norm) >= 0.0:
            raise ValueError("clip_norm must be >= 0 (0: no clipping), got %r" % (clip_norm,))
        self.clip_norm, self.lr_decay = float(clip_norm), _check_decay(lr_decay)
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("MultiTensorAdam: no parameter requires a gradient")
        dev = self.params[0].device
        if dev.type != "cuda" or any(p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() for p in self.params):
            raise RuntimeError("MultiTensorAdam: heterofusionrcnn_amd has no CPU implementation (contiguous fp32 parameters on one GPU)")
        self.lr, self.betas, self.eps, self.tf_epsilon, self.grad_scale = float(lr), betas, float(eps), tf_epsilon, float(grad_scale)
        total = sum(p.numel() for p in self.params)
        # both moments of every tensor in two flat buffers, 16-byte aligned slices
        offs, o = [], 0
        for p in self.params:
            offs.append(o)
            o += (p.numel() + 3) // 4 * 4
        self._exp_avg = torch.zeros(o, dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(o, dtype=torch.float32, device=dev)
        self.exp_avg = [self._exp_avg[a:a + p.numel()] for a, p in zip(offs, self.params)]
        self.exp_avg_sq = [self._exp_avg_sq[a:a + p.numel()] for a, p in zip(offs, self.params)]
        self.step_count = torch.zeros((), dtype=torch.float32, device=dev)     # on the device: a captured step advances it
        self.chunk = _lib.lib().hf_adam_chunk()
        n = len(self.params)
        self._table_bytes = n * ctypes.sizeof(_Entry)
        self._map_rows = sum((p.numel() + self.chunk - 1) // self.chunk for p in self.params)
        # pinned staging for the table upload.  The upload is asynchronous and the host may be several steps ahead of the device,
        # so a rewrite never touches a buffer whose upload may still be pending: eager rewrites rotate through a ring (an event
        # per slot, waited on before the slot is reused); a capture takes a slot of its own for good (the graph's upload nodes
        # re-read it at every replay), together with a device table and map of its own (module docstring).  All pinned
        # allocations happen outside captures (hipHostMalloc is not capturable), the captures' device tables with them.
        self._ring = [self._new_staging() for _ in range(4)]
        self._ring_at = 0
        self._for_captures = [self._new_capture_set() for _ in range(2)]
        self._captured = []                                   # the sets captures took: alive as long as the optimizer
        self._dev_table, self._dev_map = self._new_device_table()        # the eager steps' own
        self._key, self._chunks = None, 0                     # what the last eager upload wrote there
        self.table_uploads = 0
        self.total_elements = total
        # the per-chunk sums of squares of the clipped step (one double per map row), allocated here: never inside a capture
        self._partials = torch.empty(max(self._map_rows, 1), dtype=torch.float64, device=dev)

    def _new_staging(self):
        return [torch.empty(self._table_bytes, dtype=torch.uint8).pin_memory(),
                torch.empty((self._map_rows, 2), dtype=torch.int32).pin_memory(), None]

    def _new_device_table(self):
        dev = self.params[0].device
        return (torch.empty(self._table_bytes, dtype=torch.uint8, device=dev),
                torch.empty((self._map_rows, 2), dtype=torch.int32, device=dev))

    def _new_capture_set(self):
        """what one capture owns: pinned staging, a device table and a device map"""
        return self._new_staging()[:2] + list(self._new_device_table())

    # the framework optimizers' surface that callers here use
    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _write_table(self, host_table, host_map, dev_table, dev_map):
        """the table of the tensors that have a gradient now -> pinned staging -> device, on the current stream; returns its chunks"""
        entries = (_Entry * len(self.params)).from_buffer(host_table.numpy())
        rows, live = [], 0
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or not g.is_contiguous() or g.device != p.device:
                raise RuntimeError("MultiTensorAdam: gradients must be contiguous fp32 on the parameters' device")
            entries[live] = _Entry(p.data_ptr(), g.data_ptr(), self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr(), p.numel())
            rows += [(live, c) for c in range((p.numel() + self.chunk - 1) // self.chunk)]
            live += 1
        if rows:
            host_map[:len(rows)] = torch.tensor(rows, dtype=torch.int32)
        # inside a capture the two copies become nodes of the graph: they re-upload the same bytes at every replay, 12 KB
        dev_table.copy_(host_table, non_blocking=True)
        dev_map.copy_(host_map, non_blocking=True)
        self.table_uploads += 1
        return len(rows)

    def _refresh(self):
        """-> (device table, device map, chunks) this step launches on.  Eager: the eager table, rewritten + uploaded when a gradient
        moved (or appeared / vanished) since the last eager upload.  Capturing: a table of the capture's own, always uploaded"""
        if torch.cuda.is_current_stream_capturing():
            if not self._for_captures:
                raise RuntimeError("MultiTensorAdam: no pinned staging left for another capture (run one eager step between captures)")
            own = self._for_captures.pop()
            self._captured.append(own)
            return own[2], own[3], self._write_table(*own)
        while len(self._for_captures) < 2:
            self._for_captures.append(self._new_capture_set())
        key = tuple(p.grad.data_ptr() if p.grad is not None else 0 for p in self.params)
        if key != self._key:
            slot = self._ring[self._ring_at]
            self._ring_at = (self._ring_at + 1) % len(self._ring)
            if slot[2] is not None:
                slot[2].synchronize()           # the upload that last read this slot has executed (four rewrites ago: rarely waits)
            self._key = None                    # until the upload below is enqueued the table matches no key
            self._chunks = self._write_table(slot[0], slot[1], self._dev_table, self._dev_map)
            slot[2] = torch.cuda.Event()
            slot[2].record()
            self._key = key
        return self._dev_table, self._dev_map, self._chunks

    @torch.no_grad()
    def step(self):
        table, chunk_map, chunks = self._refresh()
        self.step_count.add_(1.0)
        L = _lib.lib()
        mode = 0 if self.tf_epsilon else 1
        if self.clip_norm == 0.0 and self.lr_decay is None:
            check(L.hf_adam_multi(chunks, ptr(table), ptr(chunk_map), ptr(self.step_count), self.lr,
                                  self.betas[0], self.betas[1], self.eps, self.grad_scale, mode, stream_ptr()), "adam_multi")
            return
        # _partials is scratch of one step (written, then read, in stream order): eager and captured steps share it
        if self.clip_norm > 0.0:
            check(L.hf_adam_sqnorm_partials(chunks, ptr(table), ptr(chunk_map), self.grad_scale,
                                            ptr(self._partials), stream_ptr()), "adam_sqnorm_partials")
        decay, steps, factor = 0, 1.0, 1.0
        if self.lr_decay is not None:
            steps, factor, staircase = self.lr_decay
            decay = 2 if staircase else 1
        check(L.hf_adam_multi_sched(chunks, ptr(table), ptr(chunk_map), ptr(self.step_count), ptr(self._partials),
                                    self.clip_norm, self.lr, decay, steps, factor, self.betas[0], self.betas[1], self.eps,
                                    self.grad_scale, mode, stream_ptr()), "adam_multi_sched")

    def lr_at(self, global_step):
        """the learning rate of the update at `global_step` (= Adam step global_step + 1), computed on the host: log lines"""
        return lr_at(self.lr, self.lr_decay, global_step)

    # ---- checkpoints ----
    def _fingerprint(self):
        return {"count": len(self.params), "shapes": [tuple(int(d) for d in p.shape) for p in self.params]}

    def hyper_parameters(self):
        """the settings a checkpoint records (grad_scale is not one: the exchange of the train step sets it)"""
        return {"lr": self.lr, "betas": tuple(float(b) for b in self.betas), "eps": self.eps, "tf_epsilon": bool(self.tf_epsilon),
                "clip_norm": self.clip_norm, "lr_decay": self.lr_decay}

    def state_dict(self):
        """copies (on the parameters' device) of the flat moments and the step counter, the hyper-parameters, the fingerprint;
        enqueued on the current stream, no synchronisation"""
        return {"exp_avg": self._exp_avg.detach().clone(), "exp_avg_sq": self._exp_avg_sq.detach().clone(),
                "step_count": self.step_count.detach().clone(), "hyper_parameters": self.hyper_parameters(),
                "fingerprint": self._fingerprint()}

    def load_state_dict(self, state):
        """copy a state_dict() into this optimizer's buffers in place (a captured step keeps reading them); ValueError when the
        parameter list differs in count or shapes"""
        fp, mine = state["fingerprint"], self._fingerprint()
        if int(fp["count"]) != mine["count"] or [tuple(s) for s in fp["shapes"]] != mine["shapes"]:
            raise ValueError("MultiTensorAdam.load_state_dict: the state holds %d tensors %s, this optimizer %d %s" % (
                int(fp["count"]), _shape_summary(fp["shapes"]), mine["count"], _shape_summary(mine["shapes"])))
        if state["exp_avg"].numel() != self._exp_avg.numel() or state["exp_avg_sq"].numel() != self._exp_avg_sq.numel():
            raise ValueError("MultiTensorAdam.load_state_dict: moment buffers of the wrong length")
        with torch.no_grad():
            self._exp_avg.copy_(state["exp_avg"])
            self._exp_avg_sq.copy_(state["exp_avg_sq"])
            self.step_count.copy_(state["step_count"].reshape(()))
        hp = state["hyper_parameters"]
        self.lr, self.betas, self.eps, self.tf_epsilon = float(hp["lr"]), tuple(hp["betas"]), float(hp["eps"]), bool(hp["tf_epsilon"])
        self.clip_norm, self.lr_decay = float(hp["clip_norm"]), _check_decay(hp["lr_decay"])

    # ---- state hand-over (graph_step.TrainStep undoes its warm-up steps with these) ----
    def snapshot(self):
        return (self._exp_avg.clone(), self._exp_avg_sq.clone(), self.step_count.clone())

    def restore(self, snap):
        self._exp_avg.copy_(snap[0])
        self._exp_avg_sq.copy_(snap[1])
        self.step_count.copy_(snap[2])


def _shape_summary(shapes):
    shapes = [tuple(s) for s in shapes]
    return "(%s%s)" % (", ".join(str(s) for s in shapes[:4]), ", ..." if len(shapes) > 4 else "")
