"""Case tables, references and bounds of the image pyramid's kernels (csrc/conv_nhwc.hip: hf_conv3x3_nhwc, hf_upconv3x3s2_nhwc,
hf_maxpool2x2_nhwc) and of image_pyramid.pack / forward_native.  tests/test_image_pyramid_cases_cpu.py checks this module on any
machine, tests/test_image_pyramid_abi.py runs the cases on the GPU through the C ABI, tests/test_image_pyramid.py goes through the
Python layer.  A plain helper module: the references come from the formulas of include/hfops.h, never from the kernels.

References.  An explicit fp64 sum over taps in NHWC:
  convolution      z[p, :] = sum_t x'[oy + ky - 1, ox + kx - 1, :] wt[t]^T, t = 3 ky + kx, x' = x - in_sub inside the image and zero
                   in the padding (the subtraction is NOT applied to the padding)
  up-convolution   input pixel iy adds x[iy, ix, :] wt[t]^T to output (2 iy - 1 + ky, 2 ix - 1 + kx) where that exists
  pool             the maximum of the four pixels (2 oy + {0, 1}, 2 ox + {0, 1}); a last odd row or column is dropped
  epilogue         y = z scale + shift, max(., 0) with relu, written to columns [y_col, y_col + cout) of rows y_stride wide
Next to z the reference forms S = sum |x'| |wt| over the same taps.

Bound per output element, derived, not measured (u = 2^-24): the kernel rounds x - in_sub once (relative u, inside S to first
order: counted as one of the "+ 2"), forms every product exactly or with one rounding and adds at most 9 cin terms in some order:
|z_got - z| <= (9 cin + 2) u S for ANY summation order.  The epilogue multiplies and adds with one rounding each:
|y_got - y| <= |scale| (9 cin + 2) u S + 2 u (|scale z| + |shift|), plus a floor of 2^-120 for results in the denormal range.
max(., 0) is 1-Lipschitz: the bound holds after it unchanged.  The up-convolution has at most 4 cin terms; it keeps 9 cin.

Inputs of a case are seeded by its name."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FLOOR = 2.0 ** -120

# flags of a convolution case, cycled over the geometry table so that every combination of (shape, cin, cout) runs and every flag
# pattern meets every shape, cin and cout: (in_sub, scale and shift, relu, written into a slice)
FLAG_PATTERNS = ((1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 1), (1, 1, 0, 0))      # five: coprime to the 3 couts and 4 cins
CONV_SHAPES = ((2, 5, 7), (1, 12, 22), (3, 1, 1))        # 70 rows with an image boundary inside; two tiles and a part; one pixel each
CONV_CIN = (3, 36, 64, 256)                              # tails of the 32-wide stage and of the float4 path
CONV_COUT = (32, 40, 256)


def _conv_cases():
    cases, i = {}, 0
    for b, h, w in CONV_SHAPES:
        for cin in CONV_CIN:
            for cout in CONV_COUT:
                sub, affine, relu, sl = FLAG_PATTERNS[i % len(FLAG_PATTERNS)]
                i += 1
                cases["b%dh%dw%d_ci%d_co%d" % (b, h, w, cin, cout)] = dict(b=b, h=h, w=w, cin=cin, cout=cout, sub=bool(sub),
                                                                            affine=bool(affine), relu=bool(relu), slice=bool(sl))
    # the first layer's shape (cin = 3, the scalar path, one stage for all nine taps) with every flag pattern
    for j, (sub, affine, relu, sl) in enumerate(FLAG_PATTERNS):
        cases["first_layer_%d" % j] = dict(b=2, h=5, w=7, cin=3, cout=32, sub=bool(sub), affine=bool(affine), relu=bool(relu),
                                           slice=bool(sl))
    return cases


CONV_CASES = _conv_cases()
# all four parity classes are present in every case; always into a slice, with scale, shift and relu
UPCONV_CASES = {"b%dh%dw%d_ci%d_co%d" % (b, h, w, cin, cout): dict(b=b, h=h, w=w, cin=cin, cout=cout, sub=False, affine=True, relu=True,
                                                                    slice=True)
                for b, h, w in ((2, 3, 5), (1, 1, 1)) for cin in (36, 256) for cout in (32, 128)}
# (b, h, w, c): read from a slice (x_stride = 2 c + 4, x_col = c), and dense for the first
POOL_CASES = {"b%dh%dw%d_c%d" % (b, h, w, c): dict(b=b, h=h, w=w, c=c) for b, h, w in ((2, 6, 10), (1, 5, 7)) for c in (3, 32, 40)}


def slice_of(case):
    """(y_stride, y_col) of a case's output"""
    return (2 * case["cout"] + 4, case["cout"]) if case["slice"] else (case["cout"], 0)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def conv_inputs(kind, name):
    """float32 arrays, read-only: x (b,h,w,cin), wt (9,cout,cin), in_sub (cin) or None, scale / shift (cout) or None"""
    c = (CONV_CASES if kind == "conv" else UPCONV_CASES)[name]
    rng = _rng(kind + name)
    x = rng.uniform(-2.0, 2.0, (c["b"], c["h"], c["w"], c["cin"])).astype(np.float32)
    wt = (rng.standard_normal((9, c["cout"], c["cin"])) / np.sqrt(9.0 * c["cin"])).astype(np.float32)
    in_sub = rng.uniform(-1.0, 1.0, (c["cin"],)).astype(np.float32) if c["sub"] else None
    scale = (rng.uniform(0.5, 1.5, (c["cout"],)) * rng.choice([-1.0, 1.0], (c["cout"],))).astype(np.float32) if c["affine"] else None
    shift = rng.standard_normal((c["cout"],)).astype(np.float32) if c["affine"] else None
    for a in (x, wt, in_sub, scale, shift):
        if a is not None:
            a.flags.writeable = False
    return {"x": x, "wt": wt, "in_sub": in_sub, "scale": scale, "shift": shift}


@functools.lru_cache(maxsize=None)
def pool_inputs(name):
    c = POOL_CASES[name]
    x = _rng("pool" + name).standard_normal((c["b"], c["h"], c["w"], c["c"])).astype(np.float32)
    x.flags.writeable = False
    return x


def _t64(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64))      # a copy: the inputs are read-only


# ------------------------------------------------------------------------------------------------ the tap sums
def conv_tap_sum(x, wt, in_sub=None):
    """x (b,h,w,cin), wt (9,cout,cin), fp64 tensors -> z, S (b,h,w,cout)"""
    b, h, w, cin = x.shape
    xs = x if in_sub is None else x - in_sub
    pad = torch.zeros((b, h + 2, w + 2, cin), dtype=torch.float64)
    pad[:, 1:h + 1, 1:w + 1] = xs                           # the padding stays zero: in_sub is not subtracted from it
    z = torch.zeros((b, h, w, wt.shape[1]), dtype=torch.float64)
    s = torch.zeros_like(z)
    for ky in range(3):
        for kx in range(3):
            src = pad[:, ky:ky + h, kx:kx + w]              # pixel (oy + ky - 1, ox + kx - 1)
            z += src @ wt[3 * ky + kx].T
            s += src.abs() @ wt[3 * ky + kx].abs().T
    return z, s


def upconv_tap_sum(x, wt):
    """x (b,h,w,cin), wt (9,cout,cin) -> z, S (b,2h,2w,cout): input pixel iy feeds output row 2 iy - 1 + ky"""
    b, h, w, _ = x.shape
    z = torch.zeros((b, 2 * h, 2 * w, wt.shape[1]), dtype=torch.float64)
    s = torch.zeros_like(z)
    for ky in range(3):
        for kx in range(3):
            iy = torch.arange(1 if ky == 0 else 0, h)       # 2 iy - 1 + ky >= 0; it is <= 2 h - 1 for every iy
            ix = torch.arange(1 if kx == 0 else 0, w)
            if not len(iy) or not len(ix):
                continue
            src = x[:, iy][:, :, ix]
            oy, ox = (2 * iy - 1 + ky)[:, None], (2 * ix - 1 + kx)[None, :]
            z[:, oy, ox] += src @ wt[3 * ky + kx].T
            s[:, oy, ox] += src.abs() @ wt[3 * ky + kx].abs().T
    return z, s


def pool_ref(x):
    """(b,h,w,c) -> (b,h//2,w//2,c), any dtype"""
    oh, ow = x.shape[1] // 2, x.shape[2] // 2
    v = x[:, :2 * oh, :2 * ow]
    return torch.maximum(torch.maximum(v[:, 0::2, 0::2], v[:, 0::2, 1::2]), torch.maximum(v[:, 1::2, 0::2], v[:, 1::2, 1::2]))


def epilogue(z, s, cin, scale=None, shift=None, relu=False):
    """-> y, bound (the module docstring's)"""
    sc = torch.ones(z.shape[-1], dtype=torch.float64) if scale is None else scale
    sh = torch.zeros(z.shape[-1], dtype=torch.float64) if shift is None else shift
    y = z * sc + sh
    bound = sc.abs() * (9 * cin + 2) * U * s + 2 * U * ((sc * z).abs() + sh.abs()) + FLOOR
    return (y.clamp(min=0.0) if relu else y), bound


@functools.lru_cache(maxsize=None)
def conv_reference(kind, name):
    """-> {"y" (rows, cout) fp64, "bound" (rows, cout)}, rows in output pixel order"""
    c = (CONV_CASES if kind == "conv" else UPCONV_CASES)[name]
    t = conv_inputs(kind, name)
    z, s = conv_tap_sum(_t64(t["x"]), _t64(t["wt"]), _t64(t["in_sub"])) if kind == "conv" else upconv_tap_sum(_t64(t["x"]), _t64(t["wt"]))
    y, bound = epilogue(z, s, c["cin"], _t64(t["scale"]), _t64(t["shift"]), c["relu"])
    return {"y": y.reshape(-1, c["cout"]), "bound": bound.reshape(-1, c["cout"])}


# ------------------------------------------------------------------------------------------------ HF_EINVAL
def einval_calls(L, one):
    """{what: status} of calls that must return HF_EINVAL before any HIP call (fake non-null pointers, never dereferenced)"""
    def conv(b=1, h=4, w=4, cin=8, cout=32, x=one, wt=one, y=one, stride=None, col=0):
        return L.hf_conv3x3_nhwc(b, h, w, cin, cout, x, None, wt, None, None, 1, y, cout if stride is None else stride, col, None)

    def up(b=1, h=4, w=4, cin=8, cout=32, x=one, wt=one, y=one, stride=None, col=0):
        return L.hf_upconv3x3s2_nhwc(b, h, w, cin, cout, x, wt, None, None, 1, y, cout if stride is None else stride, col, None)

    def pool(b=1, h=4, w=4, c=8, x=one, y=one, stride=None, col=0):
        return L.hf_maxpool2x2_nhwc(b, h, w, c, x, c if stride is None else stride, col, y, None)

    bad = {}
    for name, f in (("conv", conv), ("upconv", up)):
        bad.update({name + ": b = 0": f(b=0), name + ": h = 0": f(h=0), name + ": w = 0": f(w=0), name + ": cin = 0": f(cin=0),
                    name + ": cout = 0": f(cout=0), name + ": cout = 257": f(cout=257), name + ": y_col < 0": f(col=-1),
                    name + ": slice past the stride": f(stride=40, col=9), name + ": stride < cout": f(stride=31),
                    name + ": no x": f(x=None), name + ": no wt": f(wt=None), name + ": no y": f(y=None),
                    name + ": b negative": f(b=-1),
                    # pixel rows are ints in the kernels (element and byte offsets are 64-bit): b h w <= INT_MAX, and a quarter of
                    # that for the up-convolution, whose output has four times the rows
                    name + ": b h w = 2^31": f(b=1 << 11, h=1 << 10, w=1 << 10)})
    bad["upconv: 4 b h w = 2^31"] = up(b=1 << 9, h=1 << 10, w=1 << 10)
    bad.update({"pool: b = 0": pool(b=0), "pool: h = 0": pool(h=0), "pool: w = 0": pool(w=0), "pool: c = 0": pool(c=0),
                "pool: x_col < 0": pool(col=-1), "pool: slice past the stride": pool(stride=12, col=5), "pool: no x": pool(x=None),
                "pool: no y": pool(y=None)})
    return bad


# ------------------------------------------------------------------------------------------------ the module
MODEL_CONV = ((1, 8), (1, 16), (2, 16), (1, 32))
MODEL_IMAGE = (2, 24, 40, 3)
MODEL_SEED = 0
TOL_MARGIN = 8               # a different fp32 summation order over the same sum lengths
SWAP_FACTOR = 10             # every swapped concat must move the fp64 output by more than this many tolerances


def make_model(seed=MODEL_SEED, conv=MODEL_CONV):
    """ImgVggPyr in eval mode on the host, fp32, with randomised gamma, beta and running statistics"""
    from heterofusionrcnn_amd.inference import ImgVggPyr
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    net = ImgVggPyr(conv)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.empty_like(m.weight).uniform_(0.5, 1.5, generator=g))
                m.bias.copy_(torch.empty_like(m.bias).normal_(0.0, 0.3, generator=g))
                m.running_mean.copy_(torch.empty_like(m.running_mean).normal_(0.0, 0.3, generator=g))
                m.running_var.copy_(torch.empty_like(m.running_var).uniform_(0.5, 1.5, generator=g))
    return net.eval()


def make_image(seed=MODEL_SEED, shape=MODEL_IMAGE):
    return torch.empty(shape).uniform_(0.0, 255.0, generator=torch.Generator().manual_seed(1000 + seed))


def module_forward(net, image, swap=None):
    """ImgVggPyr.forward restated (the default route, on the host); swap = 3, 2 or 1: the two halves of that level's concat change
    places, [up | encoder] instead of [encoder | up]"""
    from heterofusionrcnn_amd.inference import IMAGE_MEAN
    x = image.permute(0, 3, 1, 2) - torch.tensor(IMAGE_MEAN, dtype=image.dtype).view(1, 3, 1, 1)
    cat = lambda level, enc, up: torch.cat([up, enc] if swap == level else [enc, up], dim=1)
    conv1 = net.conv1(x)
    conv2 = net.conv2(F.max_pool2d(conv1, 2))
    conv3 = net.conv3(F.max_pool2d(conv2, 2))
    conv4 = net.conv4(F.max_pool2d(conv3, 2))
    f3 = net.fusion3(cat(3, conv3, net.upconv3(conv4)))
    f2 = net.fusion2(cat(2, conv2, net.upconv2(f3)))
    f1 = net.fusion1(cat(1, conv1, net.upconv1(f2)))
    return f1.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def model_reference(seed=MODEL_SEED):
    """-> {"ref64": the module's own fp64 host forward, "tol": TOL_MARGIN max|fp32 host torch route - fp64|, "fp32_err", "swaps":
    [max|swapped - ref64| for the concat of level 3, 2, 1], "max": max|ref64|}; computed once per session"""
    import copy
    net, image = make_model(seed), make_image(seed)
    with torch.no_grad():
        net64 = copy.deepcopy(net).double()
        ref64 = net64(image.double())
        err = float((net(image).double() - ref64).abs().max())
        swaps = [float((module_forward(net64, image.double(), level) - ref64).abs().max()) for level in (3, 2, 1)]
        restated = module_forward(net64, image.double())
    assert torch.equal(restated, ref64), "module_forward does not restate ImgVggPyr.forward"
    return {"ref64": ref64, "tol": TOL_MARGIN * err, "fp32_err": err, "swaps": swaps, "max": float(ref64.abs().max())}
