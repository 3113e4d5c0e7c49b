"""The image pyramid (inference.ImgVggPyr) in eval mode on this package's own channel-last kernels (csrc/conv_nhwc.hip): opt-in,
inference only.

  image_branch(mode)   with image_pyramid.image_branch("native"): ... -- ImgVggPyr.forward sends a device fp32 image to
                       forward_native for the duration; "torch" (the default) is the stock module on the vendor library, bit for bit
  pack(img_net)        per layer the (9, cout, cin) tap matrices and the eval-mode BatchNorm folded into scale / shift; cached per
                       module, rebuilt when a parameter or buffer was written or replaced
  forward_native       (B, H, W, 3) -> (B, H, W, c1): hf_conv3x3_nhwc / hf_upconv3x3s2_nhwc / hf_maxpool2x2_nhwc on three concat
                       buffers (B, H_l, W_l, 2 c_l).  The last convolution of an encoder block writes the left half of its level's
                       buffer, the pool reads that half, the up-convolution writes the right half, the fusion convolution reads the
                       whole rows: [encoder | up] is the module's order, and there is no permute and no cat.  One launch per
                       convolution, up-convolution and pool of the module, nothing else.

Training never comes here: the scope raises for a module in training mode or with autograd on."""
import functools
import weakref

import torch

from . import _lib
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


def fold_bn(bn):
    """eval-mode BatchNorm as y = z * scale + shift: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale,
    in fp64, cast to the parameters' type"""
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.double() * scale
    return scale.to(bn.weight.dtype).contiguous(), shift.to(bn.weight.dtype).contiguous()


def _pack_layer(seq):
    """_ConvBNReLU / _UpConvBNReLU -> {"wt" (9, cout, cin) with tap t = 3 ky + kx, "scale", "shift", "cin", "cout", "up"}"""
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


def _conv(layer, x, y, y_col=0, in_sub=None):
    """one launch: x (b, h, w, cin) dense -> columns [y_col, y_col + cout) of y's rows (b, h, w, y_stride), or (b, 2h, 2w, .)"""
    b, h, w, cin = x.shape
    require(cin == layer["cin"], "the layer takes %d channels, the input has %d" % (layer["cin"], cin))
    L = _lib.lib()
    if layer["up"]:
        check(L.hf_upconv3x3s2_nhwc(b, h, w, cin, layer["cout"], ptr(x), ptr(layer["wt"]), ptr(layer["scale"]), ptr(layer["shift"]), 1,
                                    ptr(y), y.shape[-1], y_col, stream_ptr()), "upconv3x3s2_nhwc")
    else:
        check(L.hf_conv3x3_nhwc(b, h, w, cin, layer["cout"], ptr(x), ptr(in_sub), ptr(layer["wt"]), ptr(layer["scale"]),
                                ptr(layer["shift"]), 1, ptr(y), y.shape[-1], y_col, stream_ptr()), "conv3x3_nhwc")
    return y


def forward_native(img_net, image):
    """ImgVggPyr.forward in eval mode on the kernels of csrc/conv_nhwc.hip: image (B, H, W, 3) fp32 on the device, H and W multiples
    of 8 (three pools and three doublings must meet again) -> (B, H, W, c1) contiguous"""
    image = _lib.dev_tensor(image, torch.float32, "image")
    require(image.dim() == 4 and image.shape[-1] == 3, "image shape must be (B, H, W, 3), got %s" % (tuple(image.shape),))
    b, h, w, _ = image.shape
    require(b > 0 and h % 8 == 0 and w % 8 == 0 and h > 0 and w > 0, "image height and width must be positive multiples of 8, got %d x %d" % (h, w))
    p = pack(img_net)
    NATIVE_CALLS[0] += 1
    L = _lib.lib()
    new = lambda hh, ww, c: torch.empty((b, hh, ww, c), dtype=torch.float32, device=image.device)
    x, sub, cats = image, p["mean"], []
    for level, block in enumerate(p["blocks"]):
        hh, ww = h >> level, w >> level
        for i, layer in enumerate(block):
            into_cat = level < 3 and i == len(block) - 1
            if into_cat:
                cats.append(new(hh, ww, 2 * layer["cout"]))          # [encoder | up]
            x = _conv(layer, x, cats[-1] if into_cat else new(hh, ww, layer["cout"]), 0, sub)
            sub = None
        if level < 3:
            c = block[-1]["cout"]
            pooled = new(hh // 2, ww // 2, c)
            check(L.hf_maxpool2x2_nhwc(b, hh, ww, c, ptr(x), 2 * c, 0, ptr(pooled), stream_ptr()), "maxpool2x2_nhwc")
            x = pooled
    for level, up, fusion in zip((2, 1, 0), p["up"], p["fusion"]):
        cat = cats[level]
        require(cat.shape[-1] == 2 * up["cout"] == fusion["cin"], "the decoder's widths do not match the encoder's")
        _conv(up, x, cat, up["cout"])
        x = _conv(fusion, cat, new(h >> level, w >> level, fusion["cout"]))
    return x
