"""The dense half of both stages: the autograd nodes, eval routes and routing decisions of the shared MLPs (tf_util.conv2d's linear +
batch_norm + relu, hf/core/feature_extractors/tf_util.py:190-203,554-581; pointnet_util.py:156-176), of their first layers on
neighbourhoods and three_nn rows read in place, of BatchNormReLU (with its fused ELU and dropout), of the tall and narrow linear layers,
and the bf16 inference and training switches of the wide ones.

This module decides which kernel a shape takes and keeps the tensors autograd needs; every launch goes through one function of
_dense_kernels.py.  No framework fallback on the GPU path: a tensor on the host raises."""
import functools
import inspect

import torch
import torch.nn as nn

from . import _dense_kernels as _k
from . import _lib
from ._dense_kernels import _STATS_GENERATION, Running, running_stats_written  # noqa: F401  (re-exported: the counter lives there)
from ._lib import check, ptr, stream_ptr
from .determinism import record as record_deterministic
from .grouping import gather_rows_grad


def _on_gpu(*tensors):
    """every entry point below hands raw device pointers to HIP kernels: a host tensor must raise, not fault"""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("heterofusionrcnn_amd.mlp: tensors must live on the GPU (there is no CPU implementation)")


_DROP_LAYERS = [0]     # BatchNormReLU modules built so far in this process (distinct dropout seeds per layer)
DROPOUT_SALT = None     # tests: a fixed salt instead of the rank (to reproduce another rank's masks in one process)


def _dropout_salt():
    """mixed into the dropout seeds: ranks share every buffer after the parameter broadcast, their masks must still differ"""
    if DROPOUT_SALT is not None:
        return int(DROPOUT_SALT)
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class _BNReLUTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, relu):
        y, mean, invstd = _k.bn_fwd_train(x, gamma, beta, Running(running_mean, running_var, eps, momentum), int(relu))
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        ctx.relu = int(relu)   # mode bits: 1 = ReLU after, 2 = ELU before
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        dx, dgamma, dbeta, _ = _k.bn_bwd(x, dy.contiguous(), gamma, beta, mean, invstd, ctx.relu)
        return dx, dgamma, dbeta, None, None, None, None, None


class _BNDropoutTrain(torch.autograd.Function):
    """dropout(bn(act(x))) as ONE node: the keep decisions are recomputed from a per-call seed in the backward passes
    (hf_bn_dropout_fwd_train / _bwd): no mask tensor, no dropout pass in either direction"""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, relu, rate, drop_state, salt):
        y, mean, invstd, seed = _k.bn_dropout_fwd(x, gamma, beta, Running(running_mean, running_var, eps, momentum), int(relu), float(rate),
                                                  int(salt), drop_state)
        ctx.save_for_backward(x, gamma, beta, mean, invstd, seed)
        ctx.relu, ctx.rate = int(relu), float(rate)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, beta, mean, invstd, seed = ctx.saved_tensors
        dx, dgamma, dbeta = _k.bn_dropout_bwd(x, dy.contiguous(), gamma, beta, mean, invstd, ctx.relu, ctx.rate, seed)
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None


def _splitk_wgrad(g, x, chunk=None):
    """dW = g^T x for tall-skinny g (R,Cout), x (R,Cin): the reduction over R split into chunks (a batched GEMM
    that fills the chip) instead of one workgroup walking all R rows (see modules._TallSkinnyLinear).
    Routes by shape from scripts/probes/wgrad_shapes_probe.py on MI355X (us; plain library GEMM / best batched split / MFMA kernel):
      (131072, 64x3) 285 / 26 / 25     (131072, 64x64) 364 / 26 / 22    (131072, 256x320) 372 / 178 (4096-row chunks) / 234
      (16384, 64x24) 115 / 25 / 15      (16384, 256x256) 102 / 27 / 32    (32768, 256x320) 141 / 50 (2048) / 90
      (1048576, 64x3) 1881 / 75 (4096) / 132                              (1048576, 64x64) 1541 / 113 / 110"""
    r = x.shape[0]
    out = g.shape[1] * x.shape[1]
    if chunk is None:
        if 512 <= r <= (1 << 18) and out <= 128 * 128:
            return linear_wgrad(g.contiguous(), x.contiguous())   # small results: the MFMA kernel cuts the rows into chunks itself
        chunk = 4096 if r >= (1 << 17) else (2048 if r >= (1 << 15) else 1024)
    if r < 8 * chunk or out > 512 * 512:
        return linear_wgrad(g.contiguous(), x.contiguous()) if 512 <= r and out <= 512 * 512 else g.t() @ x
    main = (r // chunk) * chunk
    gw = torch.bmm(g[:main].view(-1, chunk, g.shape[1]).transpose(1, 2), x[:main].view(-1, chunk, x.shape[1])).sum(dim=0)
    if main < r:
        gw = gw + g[main:].t() @ x[main:]
    return gw


class _LinearSplitK(torch.autograd.Function):
    """y = x W^T (no bias) with the weight gradient on the split-K path: a plain nn.Linear hands dW = g^T x with a
    million rows and a 64 x 3 ... 256 x 256 result to ONE library workgroup (1.45 ms for the 3 -> 64 lifting layer of an
    X-Conv); _splitk_wgrad cuts the rows into chunks that fill the chip."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        rows, cin = x.shape
        cout = weight.shape[0]
        if _mfma_forward_pays(rows, cin, cout) and cout < 128:
            # narrow outputs (the 76-value box head: 131 072 x 512 -> 76) leave the library at 15 TFLOP/s (650 us);
            # the MFMA forward kernel streams x once (its statistics epilogue is simply not used)
            return linear_bn_fwd(x, weight.contiguous(), _zeros(cout, x.device), _NO_BN, update_running=False)[0]
        return x @ weight.t()

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        dx = g @ weight if ctx.needs_input_grad[0] else None
        dw = _splitk_wgrad(g, x) if ctx.needs_input_grad[1] else None
        return dx, dw


_NO_BN = Running(None, None, 1e-5, 0.0)     # linear_bn_fwd without a BatchNorm behind it: update_running=False
_ZEROS = {}


def _zeros(n, device):
    key = (n, str(device))
    if key not in _ZEROS:
        _ZEROS[key] = torch.zeros(n, dtype=torch.float32, device=device)
    return _ZEROS[key]


class _NarrowLinear(torch.autograd.Function):
    """y = x W^T + b for a handful of outputs (the segmentation head: 256 -> 2).  The input gradient g W is a GEMM with
    an inner dimension of 2, which the library runs at 490 us for 131 072 rows; written as Cout scaled additions it is
    one streaming pass (hf_narrow_linear_dx).  Weight gradient on the split-K path."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        dx = _k.narrow_linear_dx(g, weight.contiguous(), x.shape[1]) if ctx.needs_input_grad[0] else None
        dw = _splitk_wgrad(g, x) if ctx.needs_input_grad[1] else None
        db = g.sum(0) if ctx.needs_input_grad[2] else None
        return dx, dw, db


def linear_narrow(x, weight, bias):
    """x (.., Cin) -> (.., Cout) with Cout <= 4"""
    if x.is_cuda and x.dtype == torch.float32 and weight.shape[0] <= 4 and x.numel() // x.shape[-1] >= 2048:
        y = _NarrowLinear.apply(x.reshape(-1, x.shape[-1]).contiguous(), weight, bias)
        return y.reshape(*x.shape[:-1], weight.shape[0])
    return torch.nn.functional.linear(x, weight, bias)


def linear_nobias(x, weight, allow_bf16=False):
    """x (.., Cin) @ weight (Cout, Cin)^T; tall inputs on the device take the split-K weight gradient (from 2048 rows: the
    library's plain weight-gradient GEMM is one workgroup per output tile walking every row -- 115 us for 16384 rows x 64 x 24,
    the per-layer cost of the one-frame-per-GPU step).  allow_bf16: the caller is a wide layer in training mode whose three products
    may run on the bf16 matrix cores under training_precision("bf16") (bf16_train_route decides)"""
    if allow_bf16 and bf16_train_route(x, weight):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        y = _LinearBf16Train.apply(x2 if x2.data_ptr() % 16 == 0 else x2.clone(), weight)
        return y.reshape(*x.shape[:-1], weight.shape[0])
    if x.is_cuda and x.dtype == torch.float32 and x.numel() // x.shape[-1] >= 2048:
        y = _LinearSplitK.apply(x.reshape(-1, x.shape[-1]).contiguous(), weight)
        return y.reshape(*x.shape[:-1], weight.shape[0])
    return torch.nn.functional.linear(x, weight)


def linear_wgrad(grad_z, x, in_bn=None):
    """dW (Cout, Cin) = grad_z^T x on the fp32 MFMA kernel (csrc/gemm.hip): rows cut into chunks, partial tiles
    summed in a fixed order.  in_bn = (gamma, beta, mean, invstd) of the previous layer: x is then that layer's
    pre-BN output and relu(bn(x)) is applied while it is staged."""
    _on_gpu(grad_z, x)
    return _k.linear_wgrad(grad_z, x, in_bn)


def linear_bn_fwd(x, weight, bias, bn, in_bn=None, keep_act=False, update_running=True):
    """z = act(x) W^T + b and the batch statistics of z in one MFMA pass (csrc/gemm.hip).
    Returns (z, mean, invstd, x_act); `bn` supplies eps / momentum / running buffers (updated in place).
    in_bn = (gamma, beta, mean, invstd) of the previous layer: x is that layer's pre-BN output and relu(bn(x)) is
    applied on load; keep_act also stores that activated input (x_act, else None); update_running=False leaves the
    running estimates alone (inference: the returned batch statistics are then simply not used)."""
    _on_gpu(x, weight, bias)
    return _k.linear_bn_fwd(x, weight, bias, bn, in_bn, keep_act, update_running)


# The MFMA forward pays off where the layer is bound by memory traffic: enough 128-row tiles to fill the chip and at
# most 7 accumulator tiles per wave (Cout <= 224); wider / shorter layers keep the library GEMM plus a statistics pass
# (scripts/gemm_fwd_probe.py).
FUSED_FWD_MIN_ROWS = 32768
FUSED_FWD_MAX_COUT = 224


def _mfma_forward_pays(rows, cin, cout):
    return rows >= FUSED_FWD_MIN_ROWS and cout <= FUSED_FWD_MAX_COUT and cin <= 1024


def _mfma_backward_pays(rows, cin, cout):
    # the input-gradient kernel holds Cin / 32 accumulator tiles per wave; beyond 5 it spills
    return rows >= FUSED_FWD_MIN_ROWS and cin <= 160 and cout <= 256


# ------------------------------------------------------------------------------------------------ bf16 inference
# Inference precision of the wide dense layers, process-wide: "fp32" (default: every layer as before) or "bf16" (operands
# rounded to bf16, exact products, fp32 accumulation: hf_linear_bf16_fwd_eval of csrc/linear_bf16.hip, with the layer's
# eval-mode BatchNorm pass in its epilogue).  Consulted only for a layer in eval mode, with autograd off, on the device, whose shape
# bf16_route_pays accepts: training, and a frozen BatchNorm inside a model that still trains, never see it.
PRECISIONS = ("fp32", "bf16")
_INFERENCE_PRECISION = ["fp32"]
BF16_ROUTED_CALLS = [0]      # launches of the bf16 kernel so far (tests and probes read the difference)

# The shapes the bf16 kernel takes: those where scripts/probes/bf16_linear_timing.py measured it faster than the fp32 library GEMM
# plus the BatchNorm pass by more than the spread between repeats of the latter (profiles/bf16_inference_timing.json, "kernels" /
# "routing").  That held for every GEMM shape of the two-stage batch with 2048 rows or more (2048 x 1280 x 1024: 38 us against 53;
# 409600 x 2688 x 512: 2.1 ms against 7.9) and not for 800 x 11808 x 256 (269 us against 62: seven 128-row tiles, each walking all of
# cin alone).  Nothing narrower than 228 outputs was measured: below 64 the matrix cores have little to win, so those stay fp32 too.
# cin < 32 (coordinate branches, lifting chain, the 6-channel local MLP input) stays fp32 whatever was measured.
BF16_MIN_ROWS = 2048
BF16_MIN_CIN = 32
BF16_MIN_COUT = 64


def inference_precision_name():
    return _INFERENCE_PRECISION[0]


class _PrecisionScope:
    """with mlp.inference_precision("bf16"): ... / with mlp.training_precision("bf16"): ... -- the previous setting returns on exit"""

    def __init__(self, cell, precision):
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s, got %r" % (PRECISIONS, precision))
        self.cell, self.precision = cell, precision

    def __enter__(self):
        self.previous = self.cell[0]
        self.cell[0] = self.precision
        return self

    def __exit__(self, *exc):
        self.cell[0] = self.previous
        return False


inference_precision = functools.partial(_PrecisionScope, _INFERENCE_PRECISION)


def _bf16_operands(x, weight):
    """what both bf16 routes ask of their operands: x fp32 on the device with cin columns, cin and cout multiples of 4 (16-byte rows)"""
    cout, cin = weight.shape
    return x.is_cuda and x.dtype == torch.float32 and cin % 4 == 0 and cout % 4 == 0 and x.shape[-1] == cin


def bf16_route_pays(rows, cin, cout):
    return rows >= BF16_MIN_ROWS and cin >= max(BF16_MIN_CIN, 32) and cout >= BF16_MIN_COUT


def bf16_route(x, weight):
    """does x (.., cin) times weight (cout, cin)^T take the bf16 kernel?  The caller has checked that its layer is in eval mode."""
    if _INFERENCE_PRECISION[0] != "bf16" or torch.is_grad_enabled() or not _bf16_operands(x, weight):
        return False
    cout, cin = weight.shape
    return bf16_route_pays(x.numel() // cin, cin, cout)


def _bf16_weight(weight):
    """the bf16 copy of a weight (hf_f32_to_bf16), kept on the weight tensor between calls like BatchNormReLU.eval_invstd: the key
    holds the tensor version (in-place writes, load_state_dict), the generation counter of raw-pointer writes, and the storage;
    nothing is cached while a stream capture is running (the conversion becomes a node of the graph and is replayed)."""
    capturing = torch.cuda.is_current_stream_capturing()
    key = (weight._version, _STATS_GENERATION[0], weight.device, weight.data_ptr())
    held = getattr(weight, "_hf_bf16", None) if not capturing else None
    if held is not None and held[0] == key:
        return held[1]
    wb = _k.f32_to_bf16(weight.detach().contiguous())
    if not capturing:
        weight._hf_bf16 = (key, wb)
    return wb


def linear_bf16_eval(x, weight, bias, bn, mode):
    """inference: x (rows, cin) fp32 -> (rows, cout) fp32 on the bf16 matrix cores.  bn: a BatchNormReLU in eval mode whose pass
    runs in the GEMM's epilogue (mode = (1: ReLU) | (2: ELU before the normalisation), its own flags), or None (mode 0)."""
    _on_gpu(x, weight, bias)
    assert x.dim() == 2 and (bn is not None or mode == 0)
    x, wb = x.contiguous(), _bf16_weight(weight)
    BF16_ROUTED_CALLS[0] += 1
    bn4 = (bn.weight, bn.bias, bn.running_mean, bn.eval_invstd()) if bn is not None else (None, None, None, None)
    return _k.bf16_gemm(x, wb, bias, bn4, mode)


# ------------------------------------------------------------------------------------------------ bf16 training
# Training precision of the wide dense layers, process-wide and separate from the inference switch: "fp32" (default: every layer as
# before) or "bf16" -- the three products of a layer (z = x W^T, dx = g W, dW = g^T x) with their operands rounded to bf16, exact
# products and fp32 accumulation (csrc/linear_bf16.hip, csrc/linear_bf16_train.hip).  Tensors, master weights and the optimiser stay
# fp32; the BatchNorm passes read the fp32 z as before.  Consulted only by linear_nobias, with autograd on, for a caller that allows it.
_TRAINING_PRECISION = ["fp32"]
BF16_TRAIN_ROUTED_CALLS = [0]    # forward launches of the bf16 training route so far (tests and probes read the difference)

# The shapes the training route takes: those where scripts/probes/bf16_train_linear_timing.py measured the summed trio (forward with its
# two weight conversions, input gradient, weight gradient) faster than the fp32 trio of linear_nobias by more than the spread between
# repeats of the latter (profiles/bf16_training_timing.json, "layers" / "routing"; one MI355X, medians in us, bf16 against fp32).
# All 23 permitted shapes of the rpn_multiclass step (batch 8 and one frame) and of the RCNN step with 2048 rows or more won, by 1.09x
# to 2.74x: 2048 x 1280 x 1024 136 against 149 (spread 6), 2048 x 2048 x 1024 169 against 205, 4096 x 320 x 256 55 against 75,
# 131072 x 512 x 256 370 against 784, 65536 x 2688 x 512 1377 against 3768.  Every shape with 1024 rows or fewer lost -- 1024 x 640 x 512
# 68 against 62, 1024 x 1280 x 1024 123 against 83, 512 x 2304 x 1024 169 against 86 (few 128-row tiles, each walking all of cin alone,
# and three launches of conversions and reduction that the library does not need), the short, deep 128 x 11808 x 256 304 against 72 --
# except 128 x 256 x 256 (49 against 107), which a threshold on rows cannot tell from its losing neighbours and which stays fp32.
# No permitted layer of those steps is narrower than 256 inputs or 256 outputs, so nothing narrower was measured and nothing narrower
# is routed.
BF16_TRAIN_MIN_ROWS = 2048
BF16_TRAIN_MIN_CIN = 256
BF16_TRAIN_MIN_COUT = 256


def training_precision_name():
    return _TRAINING_PRECISION[0]


training_precision = functools.partial(_PrecisionScope, _TRAINING_PRECISION)


def under_training_precision(fn):
    """decorator of a train(..., precision="fp32"): the whole call -- the capture and every step, eager ones included -- runs under
    training_precision(precision)"""
    sig = inspect.signature(fn)

    @functools.wraps(fn)
    def run(*args, **kwargs):
        bound = sig.bind(*args, **kwargs)
        bound.apply_defaults()
        with training_precision(bound.arguments["precision"]):
            return fn(*args, **kwargs)
    return run


def bf16_train_route_pays(rows, cin, cout):
    # neither kernel needs cin >= 32 (they take cin >= 4): the floor keeps the narrow layers (coordinate branches, lifting chain) fp32
    # whatever BF16_TRAIN_MIN_CIN is set to, as bf16_route_pays does for inference
    return rows >= BF16_TRAIN_MIN_ROWS and cin >= max(BF16_TRAIN_MIN_CIN, 32) and cout >= BF16_TRAIN_MIN_COUT


def bf16_train_route(x, weight):
    """does x (.., cin) times weight (cout, cin)^T, with its two gradients, take the bf16 kernels?  The caller has checked that its
    layer is in training mode and may leave fp32."""
    if _TRAINING_PRECISION[0] != "bf16" or not torch.is_grad_enabled() or not _bf16_operands(x, weight):
        return False
    cout, cin = weight.shape
    if not weight.is_cuda or weight.dtype != torch.float32 or max(cin, cout) > 32768:    # 32768: the weight-gradient kernel's limit
        return False
    return bf16_train_route_pays(x.numel() // cin, cin, cout)


def _bf16_gemm(rows, cin, cout, x, wb):
    """(rows, cin) fp32 times wb (cout, cin) bf16, transposed -> (rows, cout) fp32: the inference kernel without an epilogue.  The three
    sizes are kept for the callers that pass them (scripts/probes/bf16_train_linear_timing.py); they are read off x and wb"""
    return _k.bf16_gemm(x, wb)


def linear_bf16_wgrad(grad_z, x):
    """dW (cout, cin) = bf16(grad_z)^T bf16(x), fp32 accumulation (csrc/linear_bf16_train.hip): rows cut into chunks, partial tiles summed
    in a fixed order"""
    _on_gpu(grad_z, x)
    return _k.linear_bf16_wgrad(grad_z, x)


class _LinearBf16Train(torch.autograd.Function):
    """y = x W^T (no bias) and its two gradients on the bf16 matrix cores.  The weight changes at every step, so nothing is cached on
    it (the _hf_bf16 copy of the inference route is neither read nor written): W and W^T are converted in every forward -- inside a
    stream capture the conversions are nodes of the graph -- and the transposed copy is saved for the backward."""

    @staticmethod
    def forward(ctx, x, weight):
        rows, cin = x.shape
        cout = weight.shape[0]
        w = weight.detach().contiguous()
        wb = _k.f32_to_bf16(w)
        wtb = _k.f32_to_bf16(w, transpose=True) if ctx.needs_input_grad[0] else None
        BF16_TRAIN_ROUTED_CALLS[0] += 1
        ctx.save_for_backward(x, wtb)
        return _bf16_gemm(rows, cin, cout, x, wb)

    @staticmethod
    def backward(ctx, g):
        x, wtb = ctx.saved_tensors
        g = g.contiguous()
        if g.data_ptr() % 16:
            g = g.clone()                # a view into a larger gradient: the kernels read sixteen bytes at a time
        rows, cin = x.shape
        dx = _bf16_gemm(rows, g.shape[1], cin, g, wtb) if ctx.needs_input_grad[0] else None
        dw = linear_bf16_wgrad(g, x) if ctx.needs_input_grad[1] else None
        return dx, dw


class _SharedMLPChain(torch.autograd.Function):
    """A whole shared MLP (tf_util.conv2d([1,1], bn=True) x L, pointnet_util.py:156-160) as ONE autograd node,
    optionally ending in the max over the K grouped rows (:163-176).

    Forward: layer l runs hf_linear_bn_fwd on the PREVIOUS layer's pre-BN output -- BN affine + ReLU applied while
    the operand is staged, batch statistics of its own output taken from the accumulators -- so between two layers
    there is no statistics pass and no separate normalisation pass; the activated input is stored once (the weight
    gradient needs it).  The tail is either the fused BN+ReLU+max-pool or one BN+ReLU apply.
    Backward: per layer the fused BN backward (dz, dgamma, dbeta), split-K dW, dX = dz W."""

    @staticmethod
    def forward(ctx, x, pool_k, layers, first, *params):
        """first = (mean0, invstd0): x IS the first layer's pre-BN output (its linear ran in _GatherLinear, on neighbourhoods
        read in place); the node then starts at that layer's BatchNorm and hands dz0 back as the gradient of x"""
        n = len(layers)
        saved, cur, in_bn = [], x, None
        for li, layer in enumerate(layers):
            w, b, gamma, beta = params[4 * li:4 * li + 4]
            if li == 0 and first is not None:
                xin, z, mean, invstd = x.new_empty(0), x, first[0], first[1]
            elif _mfma_forward_pays(cur.shape[0], w.shape[1], w.shape[0]):
                z, mean, invstd, x_act = linear_bn_fwd(cur, w, b, layer.bn, in_bn, keep_act=True)
                xin = x_act if x_act is not None else cur
            else:  # library GEMM on the materialised input, statistics in their own pass
                xin = _k.bn_apply(cur, *in_bn, 1) if in_bn is not None else cur
                z = torch.addmm(b, xin, w.t())
                mean, invstd = _k.bn_stats(z, layer.bn)
            saved.append((xin, z, mean, invstd))
            cur, in_bn = z, (gamma, beta, mean, invstd)
        if pool_k:
            out, argmax = _k.bn_maxpool_fwd(cur, pool_k, *in_bn)[:2]
        else:
            out, argmax = _k.bn_apply(cur, *in_bn, 1), None
        ctx.save_for_backward(*(t for layer_saved in saved for t in layer_saved), *params, *([argmax] if argmax is not None else []))
        ctx.n, ctx.pool_k, ctx.first = n, pool_k, first is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        n, pool_k = ctx.n, ctx.pool_k
        tensors = ctx.saved_tensors
        saved = [tensors[4 * i:4 * i + 4] for i in range(n)]
        params = tensors[4 * n:8 * n]
        argmax = tensors[8 * n] if pool_k else None
        grads = [None] * (4 * n)
        dy = dout.contiguous()
        known = None  # (dgamma, dbeta) of the layer about to be processed, when the layer above already reduced them
        # A bias that feeds a batch norm has an exactly zero gradient: sum_r dz[r, c] = a_c (sum dh - R c1 - c2 sum xhat)
        # with c1 = sum dh / R and sum xhat = 0.  The column sums the kernels can also produce are rounding noise
        # around that zero (what autodiff frameworks return); the exact value is returned and the pass skipped.
        # One zero buffer for the whole node, one slice per layer.
        couts = [params[4 * i].shape[0] for i in range(n)]
        zero_bias = torch.zeros((sum(couts),), dtype=torch.float32, device=dy.device)
        for li in range(n - 1, -1, -1):
            xin, z, mean, invstd = saved[li]
            w, b, gamma, beta = params[4 * li:4 * li + 4]
            rows, cout = z.shape
            cin = w.shape[1]
            gathered = li == 0 and ctx.first                       # this layer's linear lives in _GatherLinear: stop at dz
            need_dx = (li > 0 or ctx.needs_input_grad[0]) and not gathered
            mfma = need_dx and _mfma_backward_pays(rows, cin, cout)
            dbias = zero_bias[sum(couts[:li]):sum(couts[:li + 1])]
            dz, from_dy = None, False
            if known is None:  # reduce + dx passes of the BN backward (the pooled tail has its own pair)
                if li == n - 1 and pool_k:
                    dz, dgamma, dbeta, _ = _k.bn_maxpool_bwd(z, dy, argmax, pool_k, gamma, beta, mean, invstd)
                else:
                    dz, dgamma, dbeta, _ = _k.bn_bwd(z, dy, gamma, beta, mean, invstd, 1)
            else:
                dgamma, dbeta = known
                if mfma:
                    from_dy = True  # dz is rebuilt inside the input-gradient kernel while its operand is staged
                else:
                    dz = _k.bn_bwd_dx(z, dy, gamma, beta, mean, invstd, dgamma, dbeta, 1)
            known = None
            if mfma:
                # the BN-backward sums of the layer below, (z, gamma, beta, mean, invstd), come out of this kernel's accumulators
                prev = (saved[li - 1][1], *params[4 * li - 2:4 * li], *saved[li - 1][2:4]) if li > 0 else None
                dy, dz, known = _k.linear_bn_bwd(dy if from_dy else dz, w.t().contiguous(), z, gamma, beta, mean, invstd, dgamma, dbeta,
                                                 from_dy, prev)
            elif need_dx:
                dy = dz @ w
            if gathered:
                dy = dz
                grads[0:4] = [None, None, dgamma, dbeta]
            else:
                grads[4 * li:4 * li + 4] = [_splitk_wgrad(dz, xin), dbias, dgamma, dbeta]
        return (dy if ctx.needs_input_grad[0] else None, None, None, None, *grads)


def _shared_mlp_eval(layers, x, pool_k, extra, first_done=False):
    """inference twin of _SharedMLPChain.forward: running statistics instead of batch statistics, nothing saved.
    first_done: x is already the first layer's pre-BN output (shared_mlp_grouped)"""
    cur, in_bn = x, None
    for i, layer in enumerate(layers):
        w = layer.fc.weight if (i or not extra) else torch.nn.functional.pad(layer.fc.weight, (0, extra))
        bn = layer.bn
        if i == 0 and first_done:
            z = x
        elif _mfma_forward_pays(cur.shape[0], w.shape[1], w.shape[0]):
            z = linear_bn_fwd(cur, w, layer.fc.bias, bn, in_bn, update_running=False)[0]
        else:
            xin = _k.bn_apply(cur, *in_bn, 1) if in_bn is not None else cur
            if w is layer.fc.weight and bf16_route(xin, w):
                if pool_k and i == len(layers) - 1:      # the pooling kernel normalises: the GEMM alone
                    z = linear_bf16_eval(xin, w, layer.fc.bias, None, 0)
                else:                                    # BatchNorm + ReLU in the epilogue: cur is the layer's output
                    cur, in_bn = linear_bf16_eval(xin, w, layer.fc.bias, bn, 1), None
                    continue
            else:
                z = torch.addmm(layer.fc.bias, xin, w.t())
        cur, in_bn = z, (bn.weight, bn.bias, bn.running_mean, bn.eval_invstd())
    if in_bn is None:
        return cur
    if not pool_k:
        return _k.bn_apply(cur, *in_bn, 1)
    return _k.bn_maxpool_fwd(cur, pool_k, *in_bn, want_argmax=False)[0]


def _gather_weight(w, c, xyz_first):
    """the first layer's weight (cout, 3 + c) in the reference's column order ([xyz | features], pointnet_util.py:58-60, or
    [features | xyz] in the multi-scale module, :264) -> the gathering kernels' order [features, 0.., x, y, z, 0]"""
    cfp = (c + 3) // 4 * 4
    wx, wf = (w[:, :3], w[:, 3:3 + c]) if xyz_first else (w[:, c:c + 3], w[:, :c])
    out = w.new_zeros((w.shape[0], cfp + 4))
    out[:, :c] = wf
    out[:, cfp:cfp + 3] = wx
    return out


def _ungather_weight(dw_int, c, xyz_first):
    cfp = (c + 3) // 4 * 4
    parts = [dw_int[:, cfp:cfp + 3], dw_int[:, :c]]
    return torch.cat(parts if xyz_first else parts[::-1], dim=1)


class _GatherLinear(torch.autograd.Function):
    """z0 = [points[idx] | grouped_xyz] W^T + b with the batch statistics of z0, the neighbourhoods read IN PLACE
    (hf_linear_bn_fwd_gather / hf_linear_wgrad_gather): the (B,M,K,C+3) tensor of sample_and_group is never written,
    neither for the forward GEMM nor for the weight gradient.  Returns (z0, mean, invstd); the BatchNorm that consumes them
    is the head of _SharedMLPChain (first=...)."""

    @staticmethod
    def forward(ctx, points, idx, gxyz, weight, bias, bn, xyz_first, update_running):
        b, m, k = idx.shape
        c, n_src = (points.shape[2], points.shape[1]) if points is not None else (0, 1)
        z, mean, invstd = _k.linear_bn_fwd_gather(points, idx, gxyz, _gather_weight(weight, c, xyz_first), bias, bn, update_running)
        ctx.save_for_backward(idx, gxyz, weight, *([points] if points is not None else []))
        record_deterministic(ctx)
        ctx.dims = (b, m, k, c, n_src, weight.shape[0], xyz_first)
        ctx.mark_non_differentiable(mean, invstd)
        return z, mean, invstd

    @staticmethod
    def backward(ctx, dz, _dmean, _dinvstd):
        idx, gxyz, weight, *rest = ctx.saved_tensors
        points = rest[0] if rest else None
        b, m, k, c, n_src, cout, xyz_first = ctx.dims
        dz = dz.contiguous()
        dw = _ungather_weight(_k.linear_wgrad_gather(dz, points, idx, gxyz, c, n_src), c, xyz_first)
        dpoints = None
        if points is not None and ctx.needs_input_grad[0]:
            wf = (weight[:, 3:3 + c] if xyz_first else weight[:, :c]).contiguous()
            dg = dz @ wf                                               # (rows, c): the gradient of the gathered features
            dpoints = gather_rows_grad(dg, 0, idx, n_src, c, ctx=ctx)
        # the bias feeds a BatchNorm: its gradient is exactly zero (see _SharedMLPChain.backward)
        return dpoints, None, None, dw, torch.zeros((cout,), dtype=torch.float32, device=dz.device), None, None, None


GATHER_MAX_COUT = 256           # accumulator tiles of the MFMA forward kernel
GATHER_MAX_CFEAT = 1020
# below this many feature channels the (B,M,K,C+3) tensor is a few columns wide and cheaper to write once than to gather one
# 4-byte feature per neighbour behind its index (level 1 of config 2, C = 1: +210 us in place; level 2, C = 64: equal time, -170 MB
# of traffic -- profiles/r04_sa_gather_traffic.txt)
GATHER_MIN_CFEAT = 16


def grouped_mlp_fusable(layers, points, idx, min_cfeat=0):
    """shared_mlp_grouped's conditions: BatchNorm + ReLU on every layer, on the device, first layer within the MFMA kernel's
    range (Cout <= 256), pool_k <= 255; min_cfeat: the callers that CHOOSE between the routes pass GATHER_MIN_CFEAT"""
    first = layers[0]
    c = points.shape[2] if points is not None else 0
    return (idx.is_cuda and all(l.bn is not None and l.bn.relu for l in layers) and first.fc.out_features <= GATHER_MAX_COUT
            and min_cfeat <= c <= GATHER_MAX_CFEAT and idx.shape[2] <= 255 and first.fc.in_features == c + 3)


def shared_mlp_grouped(layers, points, idx, grouped_xyz, xyz_first=True, pool=True):
    """The MLP of a set-abstraction level on neighbourhoods read in place (pointnet_util.py:42-64 + 156-176 as one chain):
    points (B,N,C) or None, idx (B,M,K) int32, grouped_xyz (B,M,K,3) centred -> (B*M, Cout) with the max over the K
    neighbours (pool) or (B*M*K, Cout).  The first layer gathers while it stages its operand; the rest is shared_mlp's chain.
    xyz_first: the reference's column order of the first weight, [xyz | features] (single-scale module) or [features | xyz]."""
    layers = list(layers)
    first, gxyz = layers[0], grouped_xyz.detach().contiguous()
    return _first_layer_then_chain("shared_mlp_grouped", layers, idx.shape[2] if pool else 0, lambda update_running: _GatherLinear.apply(
        points, idx, gxyz, first.fc.weight, first.fc.bias, first.bn, xyz_first, update_running))


class _InterpLinear(torch.autograd.Function):
    """z0 = [three_interpolate(points2, idx, weight3) | points1] W^T + b with the batch statistics of z0, the three_nn rows read
    IN PLACE (hf_linear_bn_fwd_interp / hf_linear_wgrad_interp): the (B,N,C2+C1) concat of pointnet_fp_module
    (pointnet_util.py:311-313) is never written, neither for the forward GEMM nor for the weight gradient.  The operand's column
    order is the concat's own, so the weight is only zero-padded to a multiple of 4 columns.  Returns (z0, mean, invstd); the
    BatchNorm that consumes them is the head of _SharedMLPChain (first=...).  offsets / entries: three_nn_inverse(idx, M), needed
    for the gradient of points2 only (gather form: deterministic, in the reference loop's order)."""

    @staticmethod
    def forward(ctx, points2, points1, idx, weight3, offsets, entries, weight, bias, bn, update_running):
        b, n, _ = idx.shape
        m, c2 = points2.shape[1], points2.shape[2]
        c1 = points1.shape[2] if points1 is not None else 0
        cout = weight.shape[0]
        cin = (c2 + c1 + 3) // 4 * 4
        wp = torch.nn.functional.pad(weight.detach(), (0, cin - c2 - c1)) if cin != c2 + c1 else weight.detach().contiguous()
        z, mean, invstd = _k.linear_bn_fwd_interp(points2, points1, idx, weight3, wp, bias, bn, update_running)
        ctx.save_for_backward(points2, idx, weight3, wp, *([points1] if points1 is not None else []),
                              *([offsets, entries] if offsets is not None else []))
        ctx.dims = (b, n, m, c2, c1, cout, cin, points1 is not None, offsets is not None)
        ctx.mark_non_differentiable(mean, invstd)
        return z, mean, invstd

    @staticmethod
    def backward(ctx, dz, _dmean, _dinvstd):
        L = _lib.lib()
        b, n, m, c2, c1, cout, cin, has_skip, has_inverse = ctx.dims
        points2, idx, weight3, wp, *rest = ctx.saved_tensors
        points1 = rest.pop(0) if has_skip else None
        dz = dz.contiguous()
        dw = None
        if ctx.needs_input_grad[6]:
            dwp = _k.linear_wgrad_interp(dz, points2, points1, idx, weight3, c1, cin)
            dw = dwp[:, :c2 + c1].contiguous() if cin != c2 + c1 else dwp
        need2, need1 = ctx.needs_input_grad[0], has_skip and ctx.needs_input_grad[1]
        dp2 = dp1 = None
        if need2 or need1:
            # the gradient of the operand, once for both sources: dz0 @ W[:, :c2 + c1], kept at the padded width (the weight's
            # padding columns are zero) so that the gather below reads it in 16-byte pieces
            da = dz @ wp
            if need2:
                if not has_inverse:
                    raise RuntimeError("_InterpLinear: the gradient of points2 needs the inverse index (three_nn_inverse)")
                offsets, entries = rest
                dp2 = torch.empty((b, m, c2), dtype=torch.float32, device=dz.device)
                check(L.hf_three_interpolate_concat_grad(b, n, c2, m, da.shape[1], ptr(da), ptr(weight3), ptr(offsets), ptr(entries),
                                                         ptr(dp2), stream_ptr()), "three_interpolate_concat_grad")
            if need1:
                dp1 = da.view(b, n, -1)[:, :, c2:c2 + c1]
        # the bias feeds a BatchNorm: its gradient is exactly zero (see _SharedMLPChain.backward)
        dbias = torch.zeros((cout,), dtype=torch.float32, device=dz.device) if ctx.needs_input_grad[7] else None
        return dp2, dp1, None, None, None, None, dw, dbias, None, None


INTERP_MAX_COUT = 256           # accumulator tiles of the MFMA forward kernel
INTERP_MAX_C = 1024             # each of c2 and c1 (hf_linear_bn_fwd_interp)


def interp_route_pays(rows, cin, cout, training):
    """Where modules.PointnetFPModule takes shared_mlp_interp by default (cin = C2 + C1 of the first layer).  Always: the layer's
    GEMM already ran on the MFMA forward kernel (_mfma_forward_pays), so only the source of its operand changes.  In training the
    route also replaces the layer's weight gradient by the MFMA chunk kernel, and that pays only where the materialised route ran
    that kernel too (_splitk_wgrad: results up to 128 x 128, up to 2^18 rows); wider results go to the library's batched split there,
    which is faster than the chunk kernel by more than the concat traffic costs.  Measured, forward + backward, B = 8
    (scripts/probes/fp_interp_timing.py, profiles/fp_interp_timing.json; materialised / in place, us): 131072 rows 257 -> 128:
    955 / 1090 (forward alone 353 / 303); 32768 rows 320 -> 256: 602 / 695; 32768 rows 608 -> 256: 738 / 892 -- all three lose in
    training and are excluded here; at inference the finest level (the only one within Cout <= 224) takes the route."""
    if not _mfma_forward_pays(rows, cin, cout):
        return False
    return not training or (rows <= (1 << 18) and cout * ((cin + 3) // 4 * 4) <= 128 * 128)


def interp_mlp_fusable(layers, points2, points1, idx):
    """shared_mlp_interp's conditions: BatchNorm + ReLU on every layer, fp32 tensors on the device, the first layer within the
    kernels' range (Cout <= 256, 1 <= C2 <= 1024, C1 <= 1024) and sized for the concat [interpolated | points1]"""
    layers = list(layers)
    first = layers[0]
    c2 = points2.shape[2]
    c1 = points1.shape[2] if points1 is not None else 0
    tensors = [points2, idx] + ([points1] if points1 is not None else [])
    return (all(t.is_cuda for t in tensors) and points2.dtype == torch.float32 and (points1 is None or points1.dtype == torch.float32)
            and idx.dtype == torch.int32 and all(l.bn is not None and l.bn.relu for l in layers)
            and first.fc.out_features <= INTERP_MAX_COUT and 1 <= c2 <= INTERP_MAX_C and c1 <= INTERP_MAX_C
            and first.fc.in_features == c2 + c1)


def shared_mlp_interp(layers, points2, points1, idx, weight, inverse):
    """The MLP of a feature-propagation level on three_nn rows read in place (pointnet_util.py:303-329 as one chain):
    points2 (B,M,C2) sparse features, points1 (B,N,C1) skip features or None, idx / weight (B,N,3) from three_nn and
    three_nn_weights, inverse = three_nn_inverse(idx, M) (may be None when points2 needs no gradient) -> (B*N, Cout).
    The first layer interpolates and concatenates while it stages its operand; the rest is shared_mlp's chain."""
    layers = list(layers)
    _on_gpu(points2, points1, idx, weight)
    points2 = points2.contiguous()
    points1 = points1.contiguous() if points1 is not None else None
    idx = idx.contiguous()
    weight = weight.detach().contiguous()
    inverse = [t.contiguous() for t in inverse] if inverse is not None else [None, None]
    first = layers[0]
    return _first_layer_then_chain("shared_mlp_interp", layers, 0, lambda update_running: _InterpLinear.apply(
        points2, points1, idx, weight, *(inverse if update_running else (None, None)), first.fc.weight, first.fc.bias, first.bn,
        update_running))       # inference runs without the inverse index


def _chain_params(layers, extra=0):
    """[w, b, gamma, beta] of every layer, flattened (the tensor arguments of _SharedMLPChain); extra: zero columns appended to the
    first weight, for an input the producer padded"""
    params = []
    for i, l in enumerate(layers):
        w = l.fc.weight if (i or not extra) else torch.nn.functional.pad(l.fc.weight, (0, extra))
        params += [w, l.fc.bias, l.bn.weight, l.bn.bias]
    return params


def _first_layer_then_chain(name, layers, pool_k, first_layer):
    """the shared tail of shared_mlp_grouped and shared_mlp_interp: first_layer(update_running) runs the node that reads its operand in
    place and returns (z0, mean0, invstd0); the rest is shared_mlp's chain, started at the first layer's BatchNorm"""
    if all(l.bn.training for l in layers) and torch.is_grad_enabled():
        z0, mean0, invstd0 = first_layer(True)
        return _SharedMLPChain.apply(z0, pool_k, layers, (mean0, invstd0), *_chain_params(layers))
    assert not any(l.bn.training for l in layers), "%s: training-mode BatchNorm needs autograd enabled (or call .eval())" % name
    # inference: running statistics; the first layer still reads in place (its batch statistics are simply not used)
    with torch.no_grad():
        z0, _, _ = first_layer(False)
    return _shared_mlp_eval(layers, z0, pool_k, 0, first_done=True)


def shared_mlp(layers, x, pool_k=0):
    """x (R, Cin) through `layers` (SharedMLPLayer-like: .fc, .bn with relu) -> (R, Cout), or (R / pool_k, Cout) with
    the max over each run of pool_k rows.  One fused node in training when every layer has BN+ReLU (each layer on
    the MFMA forward kernel where that pays, else library GEMM + statistics pass); otherwise layer by layer."""
    layers = list(layers)
    _on_gpu(x)
    x = x.contiguous()
    bn_relu = all(l.bn is not None and l.bn.relu for l in layers)
    pool_ok = pool_k == 0 or (pool_k <= 255 and x.shape[0] % pool_k == 0)
    fused = bn_relu and pool_ok and all(l.bn.training for l in layers)
    extra = x.shape[1] - layers[0].fc.in_features  # zero columns appended by the producer (grouping.group_concat)
    assert extra >= 0
    if fused:
        return _SharedMLPChain.apply(x, pool_k, layers, None, *_chain_params(layers, extra))
    if bn_relu and pool_ok and not torch.is_grad_enabled() and not any(l.bn.training for l in layers):
        return _shared_mlp_eval(layers, x, pool_k, extra)
    if extra:
        x = x[:, :layers[0].fc.in_features]
    for l in layers[:-1] if pool_k else layers:
        x = l(x)
    if pool_k:
        last = layers[-1]
        if last.bn is not None and last.bn.relu and pool_k <= 255:
            return linear_bn_relu_maxpool(x, last.fc.weight, last.fc.bias, last.bn, pool_k)
        x = last(x)
        return x.view(-1, pool_k, x.shape[-1]).max(dim=1).values
    return x


class _LinearBNReLU(torch.autograd.Function):
    """One autograd node for tf_util.conv2d([1,1], bn=True): z = x W^T + b; y = relu(bn(z)).
    Saves x and z only (y is never needed again); the BN backward pass also returns the column sums of dz,
    which ARE the bias gradient -- no separate reduction over the (R, Cout) gradient tensor."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, eps, momentum, relu):
        z = torch.addmm(bias, x, weight.t())
        y, mean, invstd = _k.bn_fwd_train(z, gamma, beta, Running(running_mean, running_var, eps, momentum), 1 if relu else 0)
        ctx.save_for_backward(x, weight, z, gamma, beta, mean, invstd)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, z, gamma, beta, mean, invstd = ctx.saved_tensors
        dz, dgamma, dbeta, dbias = _k.bn_bwd(z, dy.contiguous(), gamma, beta, mean, invstd, 1 if ctx.relu else 0, colsum=True)
        dx = dz @ weight if ctx.needs_input_grad[0] else None
        dw = _splitk_wgrad(dz, x)
        return dx, dw, dbias, dgamma, dbeta, None, None, None, None, None


def linear_bn_relu(x, weight, bias, bn):
    """x (R, Cin) -> relu(bn(x W^T + b)) with `bn` a BatchNormReLU module (training mode: fused node)"""
    _on_gpu(x, weight, bias)
    if bn.training:
        return _LinearBNReLU.apply(x.contiguous(), weight, bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                   bn.eps, bn.momentum, bn.relu)
    return bn(torch.addmm(bias, x, weight.t()))


class BatchNormReLU(nn.Module):
    """BatchNorm over the last dimension of (rows, C) followed by ReLU, one fused op.
    Parameter / buffer names follow nn.BatchNorm1d (weight, bias, running_mean, running_var)."""

    def __init__(self, num_features, eps=1e-3, momentum=0.1, relu=True, elu_in=False):
        """elu_in: ELU applied to the input on load (pointfly's linear -> ELU -> BatchNorm), fused into every pass"""
        super().__init__()
        self.num_features, self.eps, self.momentum, self.relu = num_features, eps, momentum, relu
        self.elu_in = elu_in
        self.weight = nn.Parameter(torch.ones(num_features))   # gamma: tf.constant_initializer(1.0)
        self.bias = nn.Parameter(torch.zeros(num_features))    # beta: 0
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self._eval_invstd = None      # (key, 1/sqrt(running_var + eps)): inference reuses it
        # fused dropout (forward(x, dropout=rate)): [base seed, forward calls so far], advanced on the device by the kernels.  The
        # base seed follows torch.manual_seed and the order in which layers are built (no draw from the generator: the initial
        # weights stay what they were); not part of the state dict.
        _DROP_LAYERS[0] += 1
        base = (torch.initial_seed() * 0x9E3779B97F4A7C15 + _DROP_LAYERS[0] * 0xBF58476D1CE4E5B9) % (1 << 62)
        self.register_buffer("drop_state", torch.tensor([base, 0], dtype=torch.int64), persistent=False)

    @property
    def mode(self):
        """the mode bits of every BatchNorm kernel: (1: ReLU after the normalisation) | (2: ELU before it)"""
        return (1 if self.relu else 0) | (2 if self.elu_in else 0)

    def train(self, mode=True):
        self._eval_invstd = None
        return super().train(mode)

    def eval_invstd(self):
        """1/sqrt(running_var + eps), kept between inference calls (two tiny kernels per layer and batch otherwise: 1800 launches
        per batch of the two-stage inference).  The key holds the tensor version (framework writes), the package-wide
        generation counter (raw-pointer writes of the training kernels: running_stats_written) and the storage; nothing is cached while a stream
        capture is running (the graph's pool memory is reused afterwards)."""
        rv = self.running_var
        if torch.cuda.is_current_stream_capturing():
            return torch.rsqrt(rv + self.eps)
        key = (rv._version, _STATS_GENERATION[0], rv.device, rv.data_ptr())
        if self._eval_invstd is None or self._eval_invstd[0] != key:
            self._eval_invstd = (key, torch.rsqrt(rv + self.eps))
        return self._eval_invstd[1]

    def forward(self, x, dropout=0.0):
        """dropout (a rate; callers pass 0 at inference): tf.layers.dropout(rate) applied to the output -- inside the normalisation
        passes when the layer normalises with batch statistics (no pass of its own, no mask tensor), by the framework's dropout
        behind the running-statistics form (a frozen BatchNorm inside a model that still trains)"""
        assert x.dim() == 2 and x.shape[1] == self.num_features
        if not x.is_cuda:
            raise RuntimeError("BatchNormReLU: heterofusionrcnn_amd has no CPU implementation")
        x = x.contiguous()
        if self.training and dropout > 0.0:
            return _BNDropoutTrain.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.eps, self.momentum,
                                         self.mode, dropout, self.drop_state, _dropout_salt())
        if self.training:
            return _BNReLUTrain.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.eps, self.momentum, self.mode)
        y = _k.bn_apply(x, self.weight, self.bias, self.running_mean, self.eval_invstd(), self.mode)
        return torch.nn.functional.dropout(y, p=dropout, training=True) if dropout > 0.0 else y


class _LinearBNReLUMaxPool(torch.autograd.Function):
    """x (G*K, Cin) -> max over the K rows of each group of relu(bn(x W^T + b)): (G, Cout).
    The tail of a set-abstraction MLP as one node; the (G*K, Cout) normalised activation and its gradient are
    never materialised (the backward pass rebuilds the one-hot dy from the stored arg-max rows)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, eps, momentum, k):
        z = torch.addmm(bias, x, weight.t())
        pooled, argmax, mean, invstd = _k.bn_maxpool_fwd(z, k, gamma, beta, bn=Running(running_mean, running_var, eps, momentum))
        ctx.save_for_backward(x, weight, z, gamma, beta, mean, invstd, argmax)
        ctx.k = k
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        x, weight, z, gamma, beta, mean, invstd, argmax = ctx.saved_tensors
        dz, dgamma, dbeta, dbias = _k.bn_maxpool_bwd(z, dpooled.contiguous(), argmax, ctx.k, gamma, beta, mean, invstd, colsum=True)
        dx = dz @ weight if ctx.needs_input_grad[0] else None
        dw = _splitk_wgrad(dz, x)
        return dx, dw, dbias, dgamma, dbeta, None, None, None, None, None


def linear_bn_relu_maxpool(x, weight, bias, bn, k):
    """x (G*K, Cin), K rows per group -> (G, Cout); `bn` a BatchNormReLU module with relu=True"""
    assert bn.relu and x.shape[0] % k == 0 and k <= 255
    _on_gpu(x, weight, bias)
    x = x.contiguous()
    if bn.training:
        return _LinearBNReLUMaxPool.apply(x, weight, bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                          bn.eps, bn.momentum, k)
    z = torch.addmm(bias, x, weight.t())
    return _k.bn_maxpool_fwd(z, k, bn.weight, bn.bias, bn.running_mean, bn.eval_invstd(), want_argmax=False)[0]
