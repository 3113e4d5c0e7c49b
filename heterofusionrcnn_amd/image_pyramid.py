"""The image pyramid (inference.ImgVggPyr) on this package's own channel-last kernels (csrc/conv_nhwc.hip): opt-in, one scope for
inference and one for training.

  image_branch(mode)   with image_pyramid.image_branch("native"): ... -- ImgVggPyr.forward sends a device fp32 image to
                       forward_native for the duration; "torch" (the default) is the stock module on the vendor library, bit for bit
  pack(img_net)        per layer the (9, cout, cin) tap matrices and the eval-mode BatchNorm folded into scale / shift; cached per
                       module, rebuilt when a parameter or buffer was written or replaced
  forward_native       (B, H, W, 3) -> (B, H, W, c1): hf_conv3x3_nhwc / hf_upconv3x3s2_nhwc / hf_maxpool2x2_nhwc on three concat
                       buffers (B, H_l, W_l, 2 c_l).  The last convolution of an encoder block writes the left half of its level's
                       buffer, the pool reads that half, the up-convolution writes the right half, the fusion convolution reads the
                       whole rows: [encoder | up] is the module's order, and there is no permute and no cat.  One launch per
                       convolution, up-convolution and pool of the module, nothing else.

  train_branch(mode)   with image_pyramid.train_branch("native"): ... -- a module in training mode with autograd on sends a device
                       fp32 image to forward_train; every other combination behaves as without the scope
  forward_train        the same buffers in training mode, one autograd node: raw convolutions and hf_bn_relu_fwd_train_ld forward;
                       hf_bn_relu_bwd_ld, the weight gradients, the forward kernels as input gradients and the pool's gradient backward.
                       No atomics: two runs from one state give the same bits

  image_precision(p)   with image_pyramid.image_precision("bf16"): ... -- forward_native sends its convolutions to the bf16
                       matrix-core kernels of csrc/conv_nhwc_bf16.hip (fp32 tensors, bf16 operands, fp32 accumulation and epilogue),
                       all but the class that bf16_conv_pays keeps on the fp32 kernel (the first layer, cin = 3, measured slower);
                       "fp32" (the default) keeps today's bits.  forward_train never reads it

image_branch alone never trains: that scope raises for a module in training mode or with autograd on."""
import functools
import weakref

import torch

from . import _dense_kernels, _lib
from ._lib import check, ptr, require, stream_ptr

IMAGE_BRANCHES = ("torch", "native")
_IMAGE_BRANCH = ["torch"]
NATIVE_CALLS = [0]           # forward_native calls so far (tests and probes read the difference)


def image_branch_name():
    return _IMAGE_BRANCH[0]


class _BranchScope:
    """with image_pyramid.image_branch("native"): ... -- the previous setting returns on exit"""

    def __init__(self, cell, mode):
        if mode not in IMAGE_BRANCHES:
            raise ValueError("image branch must be one of %s, got %r" % (IMAGE_BRANCHES, mode))
        self.cell, self.mode = cell, mode

    def __enter__(self):
        self.previous = self.cell[0]
        self.cell[0] = self.mode
        return self

    def __exit__(self, *exc):
        self.cell[0] = self.previous
        return False


image_branch = functools.partial(_BranchScope, _IMAGE_BRANCH)

IMAGE_PRECISIONS = ("fp32", "bf16")
_IMAGE_PRECISION = ["fp32"]
NATIVE_BF16_LAUNCHES = [0]   # convolution launches of forward_native that went to csrc/conv_nhwc_bf16.hip so far


def image_precision_name():
    return _IMAGE_PRECISION[0]


class _PrecisionScope(_BranchScope):
    """with image_pyramid.image_precision("bf16"): ... -- the operand precision of forward_native's convolutions; the previous
    setting returns on exit"""

    def __init__(self, cell, mode):
        if mode not in IMAGE_PRECISIONS:
            raise ValueError("image precision must be one of %s, got %r" % (IMAGE_PRECISIONS, mode))
        self.cell, self.mode = cell, mode


image_precision = functools.partial(_PrecisionScope, _IMAGE_PRECISION)


def check_precision_route(image_branch, image_precision):
    """the public entry points' rule: bf16 convolutions exist on the native route only, and asking for them elsewhere is an error,
    never a silent fp32 run"""
    if image_precision not in IMAGE_PRECISIONS:
        raise ValueError("image precision must be one of %s, got %r" % (IMAGE_PRECISIONS, image_precision))
    if image_precision == "bf16" and image_branch != "native":
        raise ValueError("image_precision='bf16' needs image_branch='native': the vendor-library route has no bf16 convolutions")

TRAIN_BRANCHES = ("torch", "native")
_TRAIN_BRANCH = ["torch"]
NATIVE_TRAIN_CALLS = [0]     # forward_train calls so far


def train_branch_name():
    return _TRAIN_BRANCH[0]


class _TrainBranchScope(_BranchScope):
    """with image_pyramid.train_branch("native"): ... -- the training direction's own scope and cell"""

    def __init__(self, mode):
        if mode not in TRAIN_BRANCHES:
            raise ValueError("image train branch must be one of %s, got %r" % (TRAIN_BRANCHES, mode))
        self.cell, self.mode = _TRAIN_BRANCH, mode


train_branch = _TrainBranchScope


def fold_bn(bn):
    """eval-mode BatchNorm as y = z * scale + shift: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale,
    in fp64, cast to the parameters' type"""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.double() * scale
    return scale.to(bn.weight.dtype).contiguous(), shift.to(bn.weight.dtype).contiguous()


def _pack_layer(seq):
    """_ConvBNReLU / _UpConvBNReLU -> {"wt" (9, cout, cin) with tap t = 3 ky + kx, "scale", "shift", "cin", "cout", "up"};
    "wt_bf16" joins on the layer's first bf16 launch (_bf16_weights)"""
    conv, bn = seq[0], seq[1]
    up = isinstance(conv, torch.nn.ConvTranspose2d)
    w = conv.weight.detach()
    # Conv2d holds (cout, cin, ky, kx), ConvTranspose2d (cin, cout, ky, kx); both become wt[3 ky + kx][co][ci]
    wt = (w.permute(2, 3, 1, 0) if up else w.permute(2, 3, 0, 1)).reshape(9, w.shape[1] if up else w.shape[0], -1).contiguous()
    scale, shift = fold_bn(bn)
    return {"wt": wt, "scale": scale, "shift": shift, "cin": wt.shape[2], "cout": wt.shape[1], "up": up}


def _state_signature(img_net):
    return tuple((t._version, t.data_ptr()) for t in list(img_net.parameters()) + list(img_net.buffers()))


_PACKED = weakref.WeakKeyDictionary()       # module -> (signature, packed)


def pack(img_net):
    """-> {"blocks": four lists of layers (conv1 .. conv4), "up": [upconv3, upconv2, upconv1], "fusion": [fusion3, fusion2,
    fusion1], "mean": the (3,) image mean}; layers as _pack_layer makes them, on the module's device.  Cached; rebuilt when the
    _version or data_ptr() of any parameter or buffer has changed (an optimizer step, load_state_dict, .to(device))"""
    from .inference import IMAGE_MEAN
    sig = _state_signature(img_net)
    hit = _PACKED.get(img_net)
    if hit is not None and hit[0] == sig:
        return hit[1]
    w0 = img_net.conv1[0][0].weight
    packed = {"blocks": [[_pack_layer(s) for s in block] for block in (img_net.conv1, img_net.conv2, img_net.conv3, img_net.conv4)],
              "up": [_pack_layer(s) for s in (img_net.upconv3, img_net.upconv2, img_net.upconv1)],
              "fusion": [_pack_layer(s) for s in (img_net.fusion3, img_net.fusion2, img_net.fusion1)],
              "mean": torch.tensor(IMAGE_MEAN, dtype=w0.dtype, device=w0.device)}
    _PACKED[img_net] = (sig, packed)
    return packed


def bf16_conv_pays(rows, cin, cout, up):
    """whether a convolution of forward_native goes to the bf16 kernels under image_precision("bf16"): rows = b h w of the grid the
    GEMM runs over, up = the up-convolution.  One class stays on the fp32 kernel: cin % 4 != 0, the scalar staging path, which in the
    pyramid is the first layer (cin = 3, K = 27).  Its single 64-wide stage is mostly past K and staging, not the MFMA, sets its pace:
    0.342 ms (p10-p90 0.341-0.344) in bf16 against 0.252 ms (0.249-0.255) on the fp32 kernel at (8, 360, 1200, 3 -> 32), while every
    layer with cin % 4 == 0 wins by 1.6x to 4.4x (scripts/probes/image_pyramid_bf16_timing.py, profiles/image_pyramid_bf16_timing.json,
    the "layers" table).  rows, cout and up do not enter: no other class lost"""
    return cin % 4 == 0


def _bf16_weights(layer):
    """the layer's tap matrices as bf16 (hf_f32_to_bf16), made on first use and kept in the packed layer: they live and die with it"""
    wb = layer.get("wt_bf16")
    if wb is None:
        wb = layer["wt_bf16"] = _dense_kernels.f32_to_bf16(layer["wt"])
    return wb


def _conv(layer, x, y, y_col=0, in_sub=None, bf16=False):
    """one launch: x (b, h, w, cin) dense -> columns [y_col, y_col + cout) of y's rows (b, h, w, y_stride), or (b, 2h, 2w, .);
    bf16: on the kernels of csrc/conv_nhwc_bf16.hip"""
    b, h, w, cin = x.shape
    require(cin == layer["cin"], "the layer takes %d channels, the input has %d" % (layer["cin"], cin))
    L = _lib.lib()
    if bf16:
        wb = _bf16_weights(layer)
        NATIVE_BF16_LAUNCHES[0] += 1
        if layer["up"]:
            check(L.hf_upconv3x3s2_nhwc_bf16(b, h, w, cin, layer["cout"], ptr(x), ptr(wb), ptr(layer["scale"]), ptr(layer["shift"]), 1,
                                             ptr(y), y.shape[-1], y_col, stream_ptr()), "upconv3x3s2_nhwc_bf16")
        else:
            check(L.hf_conv3x3_nhwc_bf16(b, h, w, cin, layer["cout"], ptr(x), ptr(in_sub), ptr(wb), ptr(layer["scale"]),
                                         ptr(layer["shift"]), 1, ptr(y), y.shape[-1], y_col, stream_ptr()), "conv3x3_nhwc_bf16")
    elif layer["up"]:
        check(L.hf_upconv3x3s2_nhwc(b, h, w, cin, layer["cout"], ptr(x), ptr(layer["wt"]), ptr(layer["scale"]), ptr(layer["shift"]), 1,
                                    ptr(y), y.shape[-1], y_col, stream_ptr()), "upconv3x3s2_nhwc")
    else:
        check(L.hf_conv3x3_nhwc(b, h, w, cin, layer["cout"], ptr(x), ptr(in_sub), ptr(layer["wt"]), ptr(layer["scale"]),
                                ptr(layer["shift"]), 1, ptr(y), y.shape[-1], y_col, stream_ptr()), "conv3x3_nhwc")
    return y


def forward_native(img_net, image, taps=None):
    """ImgVggPyr.forward in eval mode on the kernels of csrc/conv_nhwc.hip -- under image_precision("bf16") the convolutions on those
    of csrc/conv_nhwc_bf16.hip, same buffers, same launches: image (B, H, W, 3) fp32 on the device, H and W multiples
    of 8 (three pools and three doublings must meet again) -> (B, H, W, c1) contiguous.  taps: a list that receives (name, output)
    of every convolution, up-convolution and pool in launch order, the written slice of a concat buffer as a view; no launch and no
    copy is added for it"""
    image = _lib.dev_tensor(image, torch.float32, "image")
    require(image.dim() == 4 and image.shape[-1] == 3, "image shape must be (B, H, W, 3), got %s" % (tuple(image.shape),))
    b, h, w, _ = image.shape
    require(b > 0 and h % 8 == 0 and w % 8 == 0 and h > 0 and w > 0, "image height and width must be positive multiples of 8, got %d x %d" % (h, w))
    p = pack(img_net)
    NATIVE_CALLS[0] += 1
    want_bf16 = _IMAGE_PRECISION[0] == "bf16"
    bf16 = lambda layer, rows: want_bf16 and bool(bf16_conv_pays(rows, layer["cin"], layer["cout"], layer["up"]))
    L = _lib.lib()
    new = lambda hh, ww, c: torch.empty((b, hh, ww, c), dtype=torch.float32, device=image.device)

    def tap(name, out, col=0, width=None):
        if taps is not None:
            taps.append((name, out if width is None else out[..., col:col + width]))

    x, sub, cats = image, p["mean"], []
    for level, block in enumerate(p["blocks"]):
        hh, ww = h >> level, w >> level
        for i, layer in enumerate(block):
            into_cat = level < 3 and i == len(block) - 1
            if into_cat:
                cats.append(new(hh, ww, 2 * layer["cout"]))          # [encoder | up]
            x = _conv(layer, x, cats[-1] if into_cat else new(hh, ww, layer["cout"]), 0, sub, bf16(layer, b * hh * ww))
            tap("conv%d_%d" % (level + 1, i), x, 0, layer["cout"] if into_cat else None)
            sub = None
        if level < 3:
            c = block[-1]["cout"]
            pooled = new(hh // 2, ww // 2, c)
            check(L.hf_maxpool2x2_nhwc(b, hh, ww, c, ptr(x), 2 * c, 0, ptr(pooled), stream_ptr()), "maxpool2x2_nhwc")
            tap("pool%d" % (level + 1), pooled)
            x = pooled
    for level, up, fusion in zip((2, 1, 0), p["up"], p["fusion"]):
        cat = cats[level]
        require(cat.shape[-1] == 2 * up["cout"] == fusion["cin"], "the decoder's widths do not match the encoder's")
        _conv(up, x, cat, up["cout"], None, bf16(up, b * x.shape[1] * x.shape[2]))
        tap("upconv%d" % (level + 1), cat, up["cout"], up["cout"])
        x = _conv(fusion, cat, new(h >> level, w >> level, fusion["cout"]), 0, None, bf16(fusion, b * (h >> level) * (w >> level)))
        tap("fusion%d" % (level + 1), x)
    return x


# ------------------------------------------------------------------------------------------------ the training direction
def _train_layers(img_net):
    """the module's sixteen (or fewer) conv + BatchNorm layers in execution order -> [{"seq", "up", "level", "src", "dst"}]:
    src = ("image",) | ("layer", j) the dense output of layer j | ("pool", level) the pooled left half of that level's concat |
    ("cat", level) the whole concat; dst = ("dense",) | ("cat", level, half) with half 0 = encoder, 1 = up-convolution"""
    recs = []
    for level, block in enumerate((img_net.conv1, img_net.conv2, img_net.conv3, img_net.conv4)):
        for i, seq in enumerate(block):
            src = ("layer", len(recs) - 1) if i else (("pool", level - 1) if level else ("image",))
            dst = ("cat", level, 0) if level < 3 and i == len(block) - 1 else ("dense",)
            recs.append({"seq": seq, "up": False, "level": level, "src": src, "dst": dst})
    for level, up, fusion in zip((2, 1, 0), (img_net.upconv3, img_net.upconv2, img_net.upconv1),
                                 (img_net.fusion3, img_net.fusion2, img_net.fusion1)):
        recs.append({"seq": up, "up": True, "level": level, "src": ("layer", len(recs) - 1), "dst": ("cat", level, 1)})
        recs.append({"seq": fusion, "up": False, "level": level, "src": ("cat", level), "dst": ("dense",)})
    return recs


def _tap_matrices(weight, up):
    """the module's weight -> wt (9, cout, cin), tap t = 3 ky + kx (the layout of pack)"""
    return (weight.permute(2, 3, 1, 0) if up else weight.permute(2, 3, 0, 1)).reshape(9, weight.shape[1] if up else weight.shape[0], -1).contiguous()


def _scratch(like, nbytes):
    return torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=like.device) if nbytes else None


class _PyramidTrain(torch.autograd.Function):
    """ImgVggPyr in training mode as one node: forward = raw convolution into dense z, then the batch-statistics BatchNorm + ReLU
    into the layer's place (a dense tensor or a half of its level's concat buffer); backward = per layer, decoder first, the
    BatchNorm backward (dy read in place from a column slice), the weight gradient, the input gradient into the next gradient
    buffer.  Every reduction is in a fixed order: two runs from one state give the same bits.  No host synchronisation."""

    @staticmethod
    def forward(ctx, img_net, image, *params):
        L = _lib.lib()
        from .inference import IMAGE_MEAN
        from .box_codec import const_f32
        recs = _train_layers(img_net)
        b, h, w, _ = image.shape
        new = lambda hh, ww, c: torch.empty((b, hh, ww, c), dtype=torch.float32, device=image.device)
        mean_rgb = const_f32(image.device, IMAGE_MEAN)
        cats, outs = {}, []
        for i, rec in enumerate(recs):
            weight, gamma, beta = params[3 * i:3 * i + 3]
            bn, up, level = rec["seq"][1], rec["up"], rec["level"]
            wt = _tap_matrices(weight.detach(), up)
            cout, cin = wt.shape[1], wt.shape[2]
            src = rec["src"]
            if src[0] == "image":
                x = image
            elif src[0] == "layer":
                x = outs[src[1]]
            elif src[0] == "cat":
                x = cats[src[1]]
            else:
                cat = cats[src[1]]
                c = cat.shape[-1] // 2
                x = new(cat.shape[1] // 2, cat.shape[2] // 2, c)
                check(L.hf_maxpool2x2_nhwc(b, cat.shape[1], cat.shape[2], c, ptr(cat), 2 * c, 0, ptr(x), stream_ptr()), "maxpool2x2_nhwc")
            require(x.shape[-1] == cin, "layer %d takes %d channels, its input has %d" % (i, cin, x.shape[-1]))
            hi, wi = x.shape[1], x.shape[2]
            ho, wo = (2 * hi, 2 * wi) if up else (hi, wi)
            z = new(ho, wo, cout)
            if up:
                check(L.hf_upconv3x3s2_nhwc(b, hi, wi, cin, cout, ptr(x), ptr(wt), None, None, 0, ptr(z), cout, 0, stream_ptr()),
                      "upconv3x3s2_nhwc")
            else:
                check(L.hf_conv3x3_nhwc(b, hi, wi, cin, cout, ptr(x), ptr(mean_rgb) if src[0] == "image" else None, ptr(wt), None, None, 0,
                                        ptr(z), cout, 0, stream_ptr()), "conv3x3_nhwc")
            dst = rec["dst"]
            if dst[0] == "cat":
                if dst[2] == 0:
                    cats[level] = new(ho, wo, 2 * cout)                   # [encoder | up]
                ybuf, ycol = cats[level], dst[2] * cout
                require(ybuf.shape[-1] == 2 * cout and ybuf.shape[1:3] == (ho, wo), "the decoder's widths do not match the encoder's")
            else:
                ybuf, ycol = new(ho, wo, cout), 0
            rows = b * ho * wo
            require(rows > 1, "batch statistics need more than one value per channel")
            # the running statistics are updated below, with torch's unbiased variance: the kernel gets no running pointers
            ld = ybuf.shape[-1]
            _, save_mean, save_invstd = _dense_kernels.bn_fwd_train(z.view(rows, cout), gamma.detach(), beta.detach(),
                                                                    _dense_kernels.Running(None, None, bn.eps, bn.momentum), 1,
                                                                    out=ybuf.view(rows, ld)[:, ycol:ycol + cout], ld=ld)
            outs.append(ybuf if dst[0] == "dense" else None)
            rec.update(wt=wt, x=x, z=z, mean=save_mean, invstd=save_invstd, rows=rows, cin=cin, cout=cout,
                       in_sub=mean_rgb if src[0] == "image" else None)
        # running = (1 - momentum) running + momentum batch, the variance unbiased (torch.nn.BatchNorm2d); in-place torch writes, so
        # the versions that pack() keys its cache on move
        bns = [rec["seq"][1] for rec in recs]
        moms = [bn.momentum for bn in bns]
        batch_var = torch._foreach_pow([rec["invstd"] for rec in recs], -2.0)
        torch._foreach_sub_(batch_var, [bn.eps for bn in bns])
        torch._foreach_mul_(batch_var, [m * rec["rows"] / (rec["rows"] - 1.0) for m, rec in zip(moms, recs)])
        batch_mean = torch._foreach_mul([rec["mean"] for rec in recs], moms)
        torch._foreach_mul_([bn.running_mean for bn in bns], [1.0 - m for m in moms])
        torch._foreach_add_([bn.running_mean for bn in bns], batch_mean)
        torch._foreach_mul_([bn.running_var for bn in bns], [1.0 - m for m in moms])
        torch._foreach_add_([bn.running_var for bn in bns], batch_var)
        torch._foreach_add_([bn.num_batches_tracked for bn in bns], 1)
        ctx.recs, ctx.cats, ctx.batch = recs, cats, b
        ctx.save_for_backward(*params)
        return outs[-1]

    @staticmethod
    def backward(ctx, gout):
        L = _lib.lib()
        recs, cats, b, params = ctx.recs, ctx.cats, ctx.batch, ctx.saved_tensors
        gout = gout.contiguous()
        grads = [None] * len(params)
        dense = {len(recs) - 1: gout}       # layer -> the gradient of its dense output
        dcat = {}                           # level -> the gradient of its concat buffer
        for i in reversed(range(len(recs))):
            rec = recs[i]
            gamma, beta = params[3 * i + 1], params[3 * i + 2]
            x, z, up, cin, cout, rows = rec["x"], rec["z"], rec["up"], rec["cin"], rec["cout"], rec["rows"]
            dbuf, dcol = (dcat[rec["level"]], rec["dst"][2] * cout) if rec["dst"][0] == "cat" else (dense.pop(i), 0)
            ld = dbuf.shape[-1]
            dz, dgamma, dbeta, _ = _dense_kernels.bn_bwd(z.view(rows, cout), dbuf.view(rows, ld)[:, dcol:dcol + cout], gamma.detach(),
                                                         beta.detach(), rec["mean"], rec["invstd"], 1, ld=ld)
            dz = dz.view(z.shape)
            hi, wi = x.shape[1], x.shape[2]
            dwt = torch.empty_like(rec["wt"])
            if up:
                nbytes = L.hf_upconv3x3s2_nhwc_wgrad_workspace(b, hi, wi, cin, cout)
                ws = _scratch(z, nbytes)
                check(L.hf_upconv3x3s2_nhwc_wgrad(b, hi, wi, cin, cout, ptr(x), ptr(dz), ptr(dwt), ptr(ws), nbytes, stream_ptr()),
                      "upconv3x3s2_nhwc_wgrad")
                grads[3 * i] = dwt.view(3, 3, cout, cin).permute(3, 2, 0, 1).contiguous()
            else:
                nbytes = L.hf_conv3x3_nhwc_wgrad_workspace(b, hi, wi, cin, cout)
                ws = _scratch(z, nbytes)
                check(L.hf_conv3x3_nhwc_wgrad(b, hi, wi, cin, cout, ptr(x), ptr(rec["in_sub"]), ptr(dz), ptr(dwt), ptr(ws), nbytes,
                                              stream_ptr()), "conv3x3_nhwc_wgrad")
                grads[3 * i] = dwt.view(3, 3, cout, cin).permute(2, 3, 0, 1).contiguous()
            grads[3 * i + 1], grads[3 * i + 2] = dgamma, dbeta
            src = rec["src"]
            if src[0] == "image":
                continue                                                   # the first layer computes no input gradient
            dx = torch.empty_like(x)
            # dgrad: the forward kernels on dz with the weights transposed (and the taps flipped for the plain convolution), at most
            # 256 of the input's channels per launch
            wd = (rec["wt"] if up else rec["wt"].flip(0)).transpose(1, 2)                 # (9, cin, cout)
            for c0 in range(0, cin, 256):
                c1 = min(cin, c0 + 256)
                wpart = wd[:, c0:c1].contiguous()
                if up:
                    check(L.hf_conv3x3s2_nhwc(b, hi, wi, cout, c1 - c0, ptr(dz), ptr(wpart), None, None, 0, ptr(dx), cin, c0, stream_ptr()),
                          "conv3x3s2_nhwc")
                else:
                    check(L.hf_conv3x3_nhwc(b, hi, wi, cout, c1 - c0, ptr(dz), None, ptr(wpart), None, None, 0, ptr(dx), cin, c0,
                                            stream_ptr()), "conv3x3_nhwc")
            if src[0] == "layer":
                dense[src[1]] = dx
            elif src[0] == "cat":
                dcat[src[1]] = dx                                          # the whole (rows, 2 c) concat gradient
            else:
                # the pool's gradient meets the concat's in the left half of the level's gradient buffer
                cat, g = cats[src[1]], dcat[src[1]]
                c = cat.shape[-1] // 2
                check(L.hf_maxpool2x2_nhwc_bwd(b, cat.shape[1], cat.shape[2], c, ptr(cat), 2 * c, 0, ptr(dx), ptr(g), 2 * c, 0, 1,
                                               stream_ptr()), "maxpool2x2_nhwc_bwd")
        return (None, None) + tuple(grads)


def forward_train(img_net, image):
    """ImgVggPyr.forward in training mode on the kernels of csrc/conv_nhwc.hip and the BatchNorm passes of csrc/mlp.hip: image
    (B, H, W, 3) fp32 on the device, H and W multiples of 8 -> (B, H, W, c1) with a hand-written backward for every convolution
    weight, gamma and beta.  Updates running_mean, running_var and num_batches_tracked in place as the stock module does.  The
    image gets no gradient: one that requires it is refused"""
    image = _lib.dev_tensor(image, torch.float32, "image")
    require(image.dim() == 4 and image.shape[-1] == 3, "image shape must be (B, H, W, 3), got %s" % (tuple(image.shape),))
    b, h, w, _ = image.shape
    require(b > 0 and h % 8 == 0 and w % 8 == 0 and h > 0 and w > 0, "image height and width must be positive multiples of 8, got %d x %d" % (h, w))
    if image.requires_grad:
        raise RuntimeError("train_branch('native') computes no gradient for the image: it must not require one")
    params = []
    for rec in _train_layers(img_net):
        conv, bn = rec["seq"][0], rec["seq"][1]
        params += [conv.weight, bn.weight, bn.bias]
    NATIVE_TRAIN_CALLS[0] += 1
    return _PyramidTrain.apply(img_net, image, *params)
