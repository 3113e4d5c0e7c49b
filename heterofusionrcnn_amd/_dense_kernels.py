"""The launch site of every dense and BatchNorm kernel: one function per family of hf_bn_* / hf_linear_* / hf_lift_* / hf_f32_to_bf16* /
hf_narrow_linear_dx entries of the C ABI (csrc/mlp.hip, gemm.hip, fp_linear.hip, linear_bf16*.hip; include/hfops.h).

A function takes contiguous fp32 device tensors and plain numbers, allocates the outputs and the workspace its entry asks for, makes the
one call and returns the outputs.  No autograd, no routing and no validation live here (mlp.py and pointcnn.py own those, and their public
entry points refuse host tensors); the only state is the generation counter of the running statistics.  One function chooses between
two entries that compute the same gradients: lift_elu_bn_bwd, by the module switch LIFT_BWD_ONE_PASS and the entry's limit.  Conventions:
  bn       anything with .eps, .momentum, .running_mean, .running_var (a BatchNormReLU, or Running(...) inside a node that was handed
           the four separately); the running buffers are updated in place
  in_bn    (gamma, beta, mean, invstd) of the layer before, applied to the operand while it is staged, or None
  mode     BatchNormReLU.mode: (1: ReLU after the normalisation) | (2: ELU before it)"""
from collections import namedtuple

import torch

from ._lib import check, lib, ptr, stream_ptr

# The training kernels update running_mean / running_var through raw pointers, which bumps no tensor version: every function below that
# hands those pointers to a kernel calls running_stats_written(); BatchNormReLU.eval_invstd and mlp._bf16_weight key their caches on it.
_STATS_GENERATION = [0]

Running = namedtuple("Running", "running_mean running_var eps momentum")
_NO_IN_BN = (None, None, None, None)


def running_stats_written():
    _STATS_GENERATION[0] += 1


def _f32(like, *shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _ws(like, nbytes):
    return torch.empty((nbytes // 4,), dtype=torch.float32, device=like.device)


def _running_ptrs(bn, update=True):
    if not update:
        return None, None
    running_stats_written()
    return ptr(bn.running_mean), ptr(bn.running_var)


# ------------------------------------------------------------------------------------------------ BatchNorm passes (csrc/mlp.hip)
def _bn_ws(x, rows, c):
    nbytes = lib().hf_bn_workspace(rows, c)
    return _ws(x, nbytes), nbytes


def bn_fwd_train(x, gamma, beta, bn, mode, out=None, ld=None):
    """batch statistics of act(x) (rows, c) and the normalised output -> (y, mean, invstd); out / ld: y is the first c columns of a wider
    buffer whose rows are ld floats apart"""
    rows, c = x.shape
    y = torch.empty_like(x) if out is None else out
    mean, invstd = _f32(x, c), _f32(x, c)
    ws, nbytes = _bn_ws(x, rows, c)
    rm, rv = _running_ptrs(bn)
    check(lib().hf_bn_relu_fwd_train_ld(rows, c, ptr(x), ptr(gamma), ptr(beta), bn.eps, bn.momentum, rm, rv, mode, ptr(y),
                                        c if ld is None else ld, ptr(mean), ptr(invstd), ptr(ws), nbytes, stream_ptr()),
          "bn_relu_fwd_train")
    return y, mean, invstd


def bn_bwd(z, dy, gamma, beta, mean, invstd, mode, ld=None, colsum=False):
    """-> (dz, dgamma, dbeta, column sums of dz or None); ld: dy is the first c columns of a wider gradient (row stride in floats)"""
    rows, c = z.shape
    dz, dgamma, dbeta = torch.empty_like(z), torch.empty_like(gamma), torch.empty_like(beta)
    sums = torch.empty_like(beta) if colsum else None
    ws, nbytes = _bn_ws(z, rows, c)
    check(lib().hf_bn_relu_bwd_ld(rows, c, ptr(z), ptr(dy), c if ld is None else ld, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), mode,
                                  ptr(dz), ptr(dgamma), ptr(dbeta), ptr(sums), ptr(ws), nbytes, stream_ptr()), "bn_relu_bwd")
    return dz, dgamma, dbeta, sums


def bn_bwd_dx(z, dy, gamma, beta, mean, invstd, dgamma, dbeta, mode):
    """the second pass of bn_bwd alone, for a layer whose dgamma / dbeta were already reduced by the kernel above it -> dz"""
    dz = torch.empty_like(z)
    check(lib().hf_bn_relu_bwd_dx(z.shape[0], z.shape[1], ptr(z), ptr(dy), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), ptr(dgamma),
                                  ptr(dbeta), mode, ptr(dz), stream_ptr()), "bn_relu_bwd_dx")
    return dz


def bn_apply(z, gamma, beta, mean, invstd, mode):
    """the normalisation with given statistics (a batch's, or the running ones at inference) -> y"""
    y = torch.empty_like(z)
    check(lib().hf_bn_relu_fwd_eval(z.shape[0], z.shape[1], ptr(z), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), mode, ptr(y),
                                    stream_ptr()), "bn_relu_fwd_eval")
    return y


def bn_stats(z, bn):
    """batch statistics of z alone -> (mean, invstd)"""
    rows, c = z.shape
    mean, invstd = _f32(z, c), _f32(z, c)
    ws, nbytes = _bn_ws(z, rows, c)
    rm, rv = _running_ptrs(bn)
    check(lib().hf_bn_stats(rows, c, ptr(z), bn.eps, bn.momentum, rm, rv, ptr(mean), ptr(invstd), ptr(ws), nbytes, stream_ptr()),
          "bn_stats")
    return mean, invstd


def bn_dropout_fwd(x, gamma, beta, bn, mode, rate, salt, drop_state):
    """bn_fwd_train with dropout on the output; the keep decisions follow from the seed the kernel draws -> (y, mean, invstd, seed)"""
    rows, c = x.shape
    y, mean, invstd = torch.empty_like(x), _f32(x, c), _f32(x, c)
    seed = torch.empty((1,), dtype=torch.int64, device=x.device)
    ws, nbytes = _bn_ws(x, rows, c)
    rm, rv = _running_ptrs(bn)
    check(lib().hf_bn_dropout_fwd_train(rows, c, ptr(x), ptr(gamma), ptr(beta), bn.eps, bn.momentum, rm, rv, mode, rate, salt,
                                        ptr(drop_state), ptr(seed), ptr(y), ptr(mean), ptr(invstd), ptr(ws), nbytes, stream_ptr()),
          "bn_dropout_fwd_train")
    return y, mean, invstd, seed


def bn_dropout_bwd(x, dy, gamma, beta, mean, invstd, mode, rate, seed):
    """-> (dx, dgamma, dbeta)"""
    rows, c = x.shape
    dx, dgamma, dbeta = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(beta)
    ws, nbytes = _bn_ws(x, rows, c)
    check(lib().hf_bn_dropout_bwd(rows, c, ptr(x), ptr(dy), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), mode, rate, ptr(seed), ptr(dx),
                                  ptr(dgamma), ptr(dbeta), ptr(ws), nbytes, stream_ptr()), "bn_dropout_bwd")
    return dx, dgamma, dbeta


def bn_maxpool_fwd(z, k, gamma, beta, mean=None, invstd=None, bn=None, want_argmax=True):
    """max over each run of k rows of relu(bn(z)) -> (pooled, argmax or None, mean, invstd).  bn given: the batch statistics are taken
    here (and the running ones updated); else mean / invstd are the statistics to normalise with"""
    rows, c = z.shape
    pooled = _f32(z, rows // k, c)
    argmax = torch.empty((rows // k, c), dtype=torch.uint8, device=z.device) if want_argmax else None
    training, eps, momentum, rm, rv, ws, nbytes = 0, 0.0, 0.0, None, None, None, 0
    if bn is not None:
        training, eps, momentum, mean, invstd = 1, bn.eps, bn.momentum, _f32(z, c), _f32(z, c)
        ws, nbytes = _bn_ws(z, rows, c)
        rm, rv = _running_ptrs(bn)
    check(lib().hf_bn_relu_maxpool_fwd(rows // k, k, c, ptr(z), ptr(gamma), ptr(beta), training, eps, momentum, rm, rv, ptr(mean),
                                       ptr(invstd), ptr(pooled), ptr(argmax), ptr(ws), nbytes, stream_ptr()), "bn_relu_maxpool_fwd")
    return pooled, argmax, mean, invstd


def bn_maxpool_bwd(z, dpooled, argmax, k, gamma, beta, mean, invstd, colsum=False):
    """-> (dz, dgamma, dbeta, column sums of dz or None)"""
    rows, c = z.shape
    dz, dgamma, dbeta = torch.empty_like(z), torch.empty_like(gamma), torch.empty_like(beta)
    sums = torch.empty_like(beta) if colsum else None
    ws, nbytes = _bn_ws(z, rows, c)
    check(lib().hf_bn_relu_maxpool_bwd(rows // k, k, c, ptr(z), ptr(dpooled), ptr(argmax), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd),
                                       ptr(dz), ptr(dgamma), ptr(dbeta), ptr(sums), ptr(ws), nbytes, stream_ptr()), "bn_relu_maxpool_bwd")
    return dz, dgamma, dbeta, sums


# ------------------------------------------------------------------------------------------ fp32 MFMA GEMMs (csrc/gemm.hip, fp_linear.hip)
def _fwd_outputs(like, rows, cout):
    """what every GEMM with a statistics epilogue writes: z, mean, invstd, and its workspace"""
    nbytes = lib().hf_linear_bn_fwd_workspace(cout)
    return _f32(like, rows, cout), _f32(like, cout), _f32(like, cout), _ws(like, nbytes), nbytes


def _wgrad_outputs(like, rows, cout, cin):
    nbytes = lib().hf_linear_wgrad_workspace(rows, cout, cin)
    return _f32(like, cout, cin), _ws(like, nbytes), nbytes


def _bwd_ws(like, cin):
    nbytes = lib().hf_linear_bn_bwd_workspace(cin)
    return _ws(like, nbytes), nbytes


def linear_bn_fwd(x, weight, bias, bn, in_bn=None, keep_act=False, update_running=True):
    """z = act(x) W^T + b and the batch statistics of z -> (z, mean, invstd, x_act); act = relu(bn(.)) with in_bn, stored as x_act on
    keep_act (else None); update_running=False leaves the running estimates alone"""
    rows, cin = x.shape
    z, mean, invstd, ws, nbytes = _fwd_outputs(x, rows, weight.shape[0])
    g, b, m, i = in_bn if in_bn is not None else _NO_IN_BN
    x_act = torch.empty_like(x) if (keep_act and in_bn is not None) else None
    rm, rv = _running_ptrs(bn, update_running)
    check(lib().hf_linear_bn_fwd(rows, cin, weight.shape[0], ptr(x), ptr(g), ptr(b), ptr(m), ptr(i), ptr(x_act), ptr(weight), ptr(bias),
                                 ptr(z), bn.eps, bn.momentum, rm, rv, ptr(mean), ptr(invstd), ptr(ws), nbytes, stream_ptr()),
          "linear_bn_fwd")
    return z, mean, invstd, x_act


def linear_bn_bwd(g, wt, z, gamma, beta, mean, invstd, dgamma, dbeta, from_dy, prev=None):
    """dx = dz W (wt = W^T, contiguous) -> (dx, dz, (dgamma, dbeta) of the layer below or None).  from_dy: g is dy and dz, the BatchNorm
    backward of this layer, is rebuilt while the operand is staged (and returned); else g is dz.  prev = (z, gamma, beta, mean, invstd)
    of the layer below: its BatchNorm-backward sums come out of the accumulators"""
    (rows, cout), cin = z.shape, wt.shape[0]
    dx, dz = _f32(z, rows, cin), (torch.empty_like(z) if from_dy else None)
    pz = pgamma = pbeta = pmean = pinv = pdg = pdb = ws = None
    nbytes = 0
    if prev is not None:
        pz, pgamma, pbeta, pmean, pinv = prev
        pdg, pdb = torch.empty_like(pgamma), torch.empty_like(pbeta)
        ws, nbytes = _bwd_ws(z, cin)
    check(lib().hf_linear_bn_bwd(rows, cout, cin, ptr(g), ptr(z) if from_dy else None, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd),
                                 ptr(dgamma), ptr(dbeta), ptr(dz), ptr(wt), ptr(dx), ptr(pz), ptr(pgamma), ptr(pbeta), ptr(pmean),
                                 ptr(pinv), ptr(pdg), ptr(pdb), ptr(ws), nbytes, stream_ptr()), "linear_bn_bwd")
    return dx, (dz if from_dy else g), ((pdg, pdb) if prev is not None else None)


def linear_wgrad(grad_z, x, in_bn=None):
    """dW (cout, cin) = grad_z^T act(x); act = relu(bn(.)) with in_bn"""
    rows, cout = grad_z.shape
    dw, ws, nbytes = _wgrad_outputs(x, rows, cout, x.shape[1])
    g, b, m, i = in_bn if in_bn is not None else _NO_IN_BN
    check(lib().hf_linear_wgrad(rows, cout, x.shape[1], ptr(grad_z), ptr(x), ptr(g), ptr(b), ptr(m), ptr(i), ptr(dw), ptr(ws), nbytes,
                                stream_ptr()), "linear_wgrad")
    return dw


def narrow_linear_dx(g, weight, cin):
    """dx (rows, cin) = g W for a handful of outputs, as cout scaled additions"""
    dx = _f32(g, g.shape[0], cin)
    check(lib().hf_narrow_linear_dx(g.shape[0], cin, weight.shape[0], ptr(g), ptr(weight), ptr(dx), stream_ptr()), "narrow_linear_dx")
    return dx


def linear_bn_fwd_gather(points, idx, gxyz, wi, bias, bn, update_running):
    """linear_bn_fwd on [points[idx] | gxyz] read in place; wi: the weight in the kernel's column order -> (z, mean, invstd)"""
    b, m, k = idx.shape
    c, n_src = (points.shape[2], points.shape[1]) if points is not None else (0, 1)
    z, mean, invstd, ws, nbytes = _fwd_outputs(idx, b * m * k, wi.shape[0])
    rm, rv = _running_ptrs(bn, update_running)
    check(lib().hf_linear_bn_fwd_gather(b * m * k, c, wi.shape[0], ptr(points), n_src, m * k, ptr(idx), ptr(gxyz), ptr(wi), ptr(bias),
                                        ptr(z), bn.eps, bn.momentum, rm, rv, ptr(mean), ptr(invstd), ptr(ws), nbytes, stream_ptr()),
          "linear_bn_fwd_gather")
    return z, mean, invstd


def linear_wgrad_gather(dz, points, idx, gxyz, c, n_src):
    """the weight gradient of linear_bn_fwd_gather, in the kernel's column order: (cout, round_up(c, 4) + 4)"""
    b, m, k = idx.shape
    dwi, ws, nbytes = _wgrad_outputs(dz, b * m * k, dz.shape[1], (c + 3) // 4 * 4 + 4)
    check(lib().hf_linear_wgrad_gather(b * m * k, dz.shape[1], c, ptr(dz), ptr(points), n_src, m * k, ptr(idx), ptr(gxyz), ptr(dwi),
                                       ptr(ws), nbytes, stream_ptr()), "linear_wgrad_gather")
    return dwi


def linear_bn_fwd_interp(points2, points1, idx, weight3, wp, bias, bn, update_running):
    """linear_bn_fwd on [three_interpolate(points2, idx, weight3) | points1] read in place; wp: the weight zero-padded to a multiple of
    4 columns -> (z, mean, invstd)"""
    b, n, _ = idx.shape
    m, c2 = points2.shape[1], points2.shape[2]
    c1 = points1.shape[2] if points1 is not None else 0
    z, mean, invstd, ws, nbytes = _fwd_outputs(idx, b * n, wp.shape[0])
    rm, rv = _running_ptrs(bn, update_running)
    check(lib().hf_linear_bn_fwd_interp(b * n, c2, c1, wp.shape[0], ptr(points2), m, n, ptr(idx), ptr(weight3), ptr(points1), ptr(wp),
                                        ptr(bias), ptr(z), bn.eps, bn.momentum, rm, rv, ptr(mean), ptr(invstd), ptr(ws), nbytes,
                                        stream_ptr()), "linear_bn_fwd_interp")
    return z, mean, invstd


def linear_wgrad_interp(dz, points2, points1, idx, weight3, c1, cin):
    """the weight gradient of linear_bn_fwd_interp at the padded width: (cout, cin)"""
    b, n, _ = idx.shape
    dwp, ws, nbytes = _wgrad_outputs(dz, b * n, dz.shape[1], cin)
    check(lib().hf_linear_wgrad_interp(b * n, dz.shape[1], points2.shape[2], c1, ptr(dz), ptr(points2), points2.shape[1], n, ptr(idx),
                                       ptr(weight3), ptr(points1), ptr(dwp), ptr(ws), nbytes, stream_ptr()), "linear_wgrad_interp")
    return dwp


# ------------------------------------------------------------------------------------------ the lifting chain: linear -> ELU -> BatchNorm
def linear_elu_bn_fwd(x, w, bn, in_bn=None, keep_act=False):
    """z = act(x) W^T and the batch statistics of elu(z) -> (z, mean, invstd, act); act = bn(elu(.)) with in_bn, stored on keep_act"""
    rows, (cout, cin) = x.shape[0], w.shape
    z, mean, invstd, ws, nbytes = _fwd_outputs(x, rows, cout)
    act = torch.empty_like(x) if keep_act else None
    g, b, m, i = in_bn if in_bn is not None else _NO_IN_BN
    rm, rv = _running_ptrs(bn)
    check(lib().hf_linear_elu_bn_fwd(rows, cin, cout, ptr(x), ptr(g), ptr(b), ptr(m), ptr(i), ptr(act), ptr(w), ptr(z), bn.eps, bn.momentum,
                                     rm, rv, ptr(mean), ptr(invstd), ptr(ws), nbytes, stream_ptr()), "linear_elu_bn_fwd")
    return z, mean, invstd, act


def linear_elu_bn_bwd(dz1, w1t, z0, g0, b0, m0, i0):
    """dy0 = dz1 W1 (w1t = W1^T) and the BatchNorm-backward sums of the layer below from its accumulators -> (dy0, dgamma0, dbeta0)"""
    dy0, dg0, db0 = torch.empty_like(z0), torch.empty_like(g0), torch.empty_like(b0)
    ws, nbytes = _bwd_ws(z0, z0.shape[1])
    check(lib().hf_linear_elu_bn_bwd(z0.shape[0], dz1.shape[1], z0.shape[1], ptr(dz1), ptr(w1t), ptr(dy0), ptr(z0), ptr(g0), ptr(b0),
                                     ptr(m0), ptr(i0), ptr(dg0), ptr(db0), ptr(ws), nbytes, stream_ptr()), "linear_elu_bn_bwd")
    return dy0, dg0, db0


def _lift_fwd_ws(like, c0, c1):
    nbytes = lib().hf_lift_elu_bn_fwd_workspace(c0, c1)
    return _ws(like, nbytes), nbytes


def lift_elu_bn_fwd(x, w0, g0, b0, bn0, w1, bn1):
    """both layers of the chain on a 3-channel x, the first layer's output never written -> (mean0, invstd0, z1, mean1, invstd1)"""
    rows, c0, c1 = x.shape[0], w0.shape[0], w1.shape[0]
    m0, i0, m1, i1, z1 = _f32(x, c0), _f32(x, c0), _f32(x, c1), _f32(x, c1), _f32(x, rows, c1)
    ws, nbytes = _lift_fwd_ws(x, c0, c1)
    running_stats_written()
    check(lib().hf_lift_elu_bn_fwd(rows, c0, c1, ptr(x), ptr(w0), ptr(g0), ptr(b0), bn0.eps, bn0.momentum, ptr(bn0.running_mean),
                                   ptr(bn0.running_var), ptr(m0), ptr(i0), ptr(w1), ptr(z1), bn1.eps, bn1.momentum, ptr(bn1.running_mean),
                                   ptr(bn1.running_var), ptr(m1), ptr(i1), ptr(ws), nbytes, stream_ptr()), "lift_elu_bn_fwd")
    return m0, i0, z1, m1, i1


# The chain's backward with dy0 = dz1 W1 formed once (hf_onepass_lift_elu_bn_bwd, csrc/lift_bwd.hip) wherever that entry takes the shape;
# False keeps the two-pass entry everywhere.  Same dW1, dgamma0, dbeta0 bits either way; dW0 differs by fp32 rounding of its sums.
LIFT_BWD_ONE_PASS = True
LIFT_BWD_ONE_PASS_MAX_C0 = 128      # the entry's limit (include/hfops.h); wider chains take the two-pass entry


def lift_elu_bn_bwd(x, w0, g0, b0, m0, i0, dz1, w1t):
    """-> (dW0^T (3, c0), dW1, dgamma0, dbeta0)"""
    rows, c0, c1 = x.shape[0], w0.shape[0], dz1.shape[1]
    dw0_t, dw1, dg0, db0 = _f32(x, 3, c0), _f32(x, c1, c0), torch.empty_like(g0), torch.empty_like(b0)
    if LIFT_BWD_ONE_PASS and c0 <= LIFT_BWD_ONE_PASS_MAX_C0:
        nbytes = lib().hf_onepass_lift_elu_bn_bwd_workspace(rows, c0, c1)
        ws = _ws(x, nbytes)
        check(lib().hf_onepass_lift_elu_bn_bwd(rows, c0, c1, ptr(x), ptr(w0), ptr(g0), ptr(b0), ptr(m0), ptr(i0), ptr(dz1), ptr(w1t),
                                               ptr(dw0_t), ptr(dw1), ptr(dg0), ptr(db0), ptr(ws), nbytes, stream_ptr()),
              "onepass_lift_elu_bn_bwd")
        return dw0_t, dw1, dg0, db0
    nbytes = lib().hf_lift_elu_bn_bwd_workspace(rows, c0, c1)
    ws = _ws(x, nbytes)
    check(lib().hf_lift_elu_bn_bwd(rows, c0, c1, ptr(x), ptr(w0), ptr(g0), ptr(b0), ptr(m0), ptr(i0), ptr(dz1), ptr(w1t), ptr(dw0_t),
                                   ptr(dw1), ptr(dg0), ptr(db0), ptr(ws), nbytes, stream_ptr()), "lift_elu_bn_bwd")
    return dw0_t, dw1, dg0, db0


def lift_elu_fwd_eval_bn(x, w0, bn0, w1, bn1):
    """inference: both layers with given statistics, bn0 / bn1 = (gamma, beta, mean, invstd); the second layer's normalisation leaves the
    GEMM's epilogue -> the chain's output (rows, c1)"""
    rows, c0, c1 = x.shape[0], w0.shape[0], w1.shape[0]
    out = _f32(x, rows, c1)
    ws, nbytes = _lift_fwd_ws(x, c0, c1)
    check(lib().hf_lift_elu_fwd_eval_bn(rows, c0, c1, ptr(x), ptr(w0), *map(ptr, bn0), ptr(w1), *map(ptr, bn1), ptr(out), ptr(ws), nbytes,
                                        stream_ptr()), "lift_elu_fwd_eval_bn")
    return out


# ------------------------------------------------------------------------------------------------ bf16 matrix cores (csrc/linear_bf16*.hip)
def f32_to_bf16(w, transpose=False):
    """the bf16 copy of w (cout, cin), or of its transpose"""
    if transpose:
        wb = torch.empty((w.shape[1], w.shape[0]), dtype=torch.bfloat16, device=w.device)
        check(lib().hf_f32_to_bf16_transpose(w.shape[0], w.shape[1], ptr(w), ptr(wb), stream_ptr()), "f32_to_bf16_transpose")
    else:
        wb = torch.empty(w.shape, dtype=torch.bfloat16, device=w.device)
        check(lib().hf_f32_to_bf16(w.numel(), ptr(w), ptr(wb), stream_ptr()), "f32_to_bf16")
    return wb


def bf16_gemm(x, wb, bias=None, bn4=_NO_IN_BN, mode=0):
    """x (rows, cin) fp32 times wb (cout, cin) bf16, transposed -> (rows, cout) fp32; bn4 = (gamma, beta, mean, invstd): that BatchNorm's
    pass, with `mode`, in the epilogue"""
    rows, cin = x.shape
    y = _f32(x, rows, wb.shape[0])
    check(lib().hf_linear_bf16_fwd_eval(rows, cin, wb.shape[0], ptr(x), ptr(wb), ptr(bias), *map(ptr, bn4), mode, ptr(y), stream_ptr()),
          "linear_bf16_fwd_eval")
    return y


def linear_bf16_wgrad(grad_z, x):
    """dW (cout, cin) = bf16(grad_z)^T bf16(x), fp32 accumulation"""
    rows, cout = grad_z.shape
    nbytes = lib().hf_linear_bf16_wgrad_workspace(rows, cout, x.shape[1])
    ws = _ws(x, max(nbytes, 16))
    dw = _f32(x, cout, x.shape[1])
    check(lib().hf_linear_bf16_wgrad(rows, cout, x.shape[1], ptr(grad_z), ptr(x), ptr(dw), ptr(ws), nbytes, stream_ptr()),
          "linear_bf16_wgrad")
    return dw
