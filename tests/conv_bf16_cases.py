"""Case tables, references and bounds of the image pyramid's bf16 convolutions (csrc/conv_nhwc_bf16.hip: hf_conv3x3_nhwc_bf16,
hf_upconv3x3s2_nhwc_bf16).  tests/test_conv_bf16_cases_cpu.py checks this module on any machine, tests/test_conv_bf16_abi.py runs the
cases on the GPU through the C ABI, tests/test_image_pyramid_bf16.py goes through the Python layer, and
tests/test_conv_bf16_instantiations_cpu.py holds what the cases select against what the file compiles to.  A plain helper module:
the references come from the formulas of include/hfops.h, never from the kernels.

Reference (fp64 over the taps, tests/image_pyramid_cases.py: conv_tap_sum / upconv_tap_sum):
  xb = bf16_round(fl32(x - in_sub)) inside the image, zero in the padding; wb = bf16_round(wt)
  z = sum xb wb, S = sum |xb| |wb| over the taps; y = z scale + shift, max(., 0) with relu

Bound of the rounding family, derived, not measured, with u' = 2^-23 (twice the unit roundoff, so that an accumulator that truncates is
still inside): a product of two bf16 values is exact in fp32 and at most 9 cin terms are added in some order, so
|z_got - z| <= (9 cin + 8) u' S for ANY summation order; the epilogue multiplies and adds with one rounding each:
  |y_got - y| <= |scale| (9 cin + 8) u' S + 2 u' (|scale z| + |shift|) + 2^-120
max(., 0) is 1-Lipschitz: the bound carries through it.  The up-convolution has at most 4 cin terms and keeps 9 cin.

Exact family: x integers in [-8, 8], in_sub in [-2, 2], wt in [-8, 8] (|x - in_sub| <= 10 and wt are bf16 numbers), scale in
{+-1, +-2}, shift an integer: every partial sum is an integer of magnitude <= S <= 80 * 9 * 256 < 2^24 and y one of magnitude
<= 2 S + 8: fp32 numbers whatever the order.  The result equals the fp64 reference bit for bit.  exact_condition is asserted on the
reference.  This family alone reaches every instantiation of the kernel.

Dispatch, restated from launch_conv_bf16 / launch_conv_bf16_tile: the column tile is the smallest of 32, 64, 128, 256 that holds cout,
<NT, WN> = <1, 2>, <2, 2>, <4, 2>, <4, 4>; VEC where cin % 4 == 0 and x sits at a 16-byte, wt_bf16 at an 8-byte boundary; one
workgroup per 128-row tile (times four parity classes for the up-convolution): no persistent grid, so the launch regime is a grid
larger than the chip holds at once with a ragged last tile.

Inputs of a case are seeded by its name."""
import functools
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_pyramid_cases as pc  # noqa: E402
from image_pyramid_cases import FLAG_PATTERNS, conv_tap_sum, slice_of, upconv_tap_sum  # noqa: E402,F401
from linear_bf16_cases import bf16_round  # noqa: E402

U2 = 2.0 ** -23
FLOOR = 2.0 ** -120
ROW_TILE = 128                 # conv_nhwc_bf16.hip kCbRows
K_STAGE = 64                   # conv_nhwc_bf16.hip kCbKC
COL_TILES = (32, 64, 128, 256)
TILE_FORM = {32: (1, 2), 64: (2, 2), 128: (4, 2), 256: (4, 4)}      # column tile -> <NT, WN>
NUM_CU = 256

SOURCE = "conv_nhwc_bf16.hip"
SOURCE_RULES = (
    "constexpr int kCbRows = 128;",
    "constexpr int kCbKC = 64;",
    "if (cout <= 32) { HF_CONV_BF16(1, 2); }",
    "if (cout <= 64) { HF_CONV_BF16(2, 2); }",
    "if (cout <= 128) { HF_CONV_BF16(4, 2); }",
    "HF_CONV_BF16(4, 4);",
    "const bool vec = cin % 4 == 0 && bf_aligned16(x) && reinterpret_cast<uintptr_t>(wt) % 8 == 0;",
    "const dim3 grid(div_up(rows, kCbRows), UP ? 4 : 1);",
)

SHAPES = ((2, 5, 7), (1, 12, 22), (3, 1, 1))        # 70 rows with an image boundary inside a tile; two row tiles and a part; one pixel
CIN = (3, 4, 36, 64, 256)                           # scalar path; smallest vector path; K = 324, no multiple of the stage; exact stages; deepest
COUT = (1, 31, 32, 33, 40, 63, 64, 65, 127, 128, 129, 255, 256)      # below, at and above every column-tile edge
UP_SHAPES = ((2, 3, 5), (1, 1, 1))
ALIGN_COUT = (32, 40, 128, 256)                     # one per column tile


def column_tile(cout):
    return next(t for t in COL_TILES if cout <= t)


def instantiation(c):
    """the kernel a case launches; c["off"]: the operand ("x" or "wt") that sits one element past a 16-byte boundary"""
    vec = c["cin"] % 4 == 0 and c.get("off") is None
    return ("conv3x3_bf16_kernel", TILE_FORM[column_tile(c["cout"])] + (vec, c["mode"] == "up"))


def stages(c):
    """K stages of 64 per parity class (one entry for the plain form)"""
    return tuple(pc.cdiv(t * c["cin"], K_STAGE) for t in (pc.UP_CLASS_TAPS if c["mode"] == "up" else (9,)))


def workgroups(c):
    return pc.cdiv(c["b"] * c["h"] * c["w"], ROW_TILE) * (4 if c["mode"] == "up" else 1)


def _case(mode, b, h, w, cin, cout, flags, off=None):
    sub, affine, relu, sl = flags
    c = dict(mode=mode, b=b, h=h, w=w, cin=cin, cout=cout, sub=bool(sub) and mode == "conv", affine=bool(affine), relu=bool(relu),
             slice=bool(sl), off=off)
    return "b%dh%dw%d_ci%d_co%d%s" % (b, h, w, cin, cout, "_off_" + off if off else ""), c


def _table(mode, shapes, product=False):
    """every (cin, cout) of CIN x COUT once, the geometry rotating so that every cin and every cout meets every geometry -- or, with
    `product`, on every geometry; the five flag patterns cycle over the table; then, per column tile, x and wt_bf16 one element past
    a 16-byte boundary (the scalar path for alignment alone)"""
    cases, n = {}, 0
    for i, cin in enumerate(CIN):
        for j, cout in enumerate(COUT):
            for b, h, w in (shapes if product else (shapes[(i + j) % len(shapes)],)):
                name, c = _case(mode, b, h, w, cin, cout, FLAG_PATTERNS[n % len(FLAG_PATTERNS)])
                cases[name] = c
                n += 1
    b, h, w = shapes[1 if len(shapes) > 2 else 0]
    for j, cout in enumerate(ALIGN_COUT):
        for k, off in enumerate(("x", "wt")):
            name, c = _case(mode, b, h, w, 36, cout, FLAG_PATTERNS[(2 * j + k) % len(FLAG_PATTERNS)], off)
            cases[name] = c
    return cases


ROUND_CONV_CASES = _table("conv", SHAPES, product=True)
EXACT_CONV_CASES = _table("conv", SHAPES)
EXACT_UPCONV_CASES = _table("up", UP_SHAPES + ((1, 12, 22),))
# the up-convolution's rounding family: all four parity classes in every case, always into a slice, with scale, shift and relu
ROUND_UPCONV_CASES = dict(_case("up", b, h, w, cin, cout, (0, 1, 1, 1)) for b, h, w in UP_SHAPES for cin in (36, 256) for cout in (32, 128))
# exact inputs on grids larger than the chip holds at once (4099 tiles of 128 rows, the last one ragged; four times that for the
# up-convolution), image rows and image boundaries inside tiles
REGIME_CASES = {
    "conv_vec": dict(mode="conv", b=3, h=349, w=501, cin=4, cout=8, sub=True, affine=True, relu=True, slice=True, off=None),
    "conv_first_layer": dict(mode="conv", b=3, h=349, w=501, cin=3, cout=32, sub=True, affine=True, relu=True, slice=False, off=None),
    "up_vec": dict(mode="up", b=3, h=349, w=501, cin=4, cout=8, sub=False, affine=True, relu=True, slice=True, off=None),
}
TABLES = {"round": {"conv": ROUND_CONV_CASES, "up": ROUND_UPCONV_CASES}, "exact": {"conv": EXACT_CONV_CASES, "up": EXACT_UPCONV_CASES}}


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def round_inputs(name, c):
    """float32 arrays as image_pyramid_cases.conv_inputs makes them: x, wt, in_sub / scale / shift or None"""
    rng = np.random.default_rng(zlib.crc32(("bf16round" + c["mode"] + name).encode()))
    x = rng.uniform(-2.0, 2.0, (c["b"], c["h"], c["w"], c["cin"])).astype(np.float32)
    wt = (rng.standard_normal((9, c["cout"], c["cin"])) / np.sqrt(9.0 * c["cin"])).astype(np.float32)
    in_sub = rng.uniform(-1.0, 1.0, (c["cin"],)).astype(np.float32) if c["sub"] else None
    scale = (rng.uniform(0.5, 1.5, (c["cout"],)) * rng.choice([-1.0, 1.0], (c["cout"],))).astype(np.float32) if c["affine"] else None
    shift = rng.standard_normal((c["cout"],)).astype(np.float32) if c["affine"] else None
    return {"x": x, "wt": wt, "in_sub": in_sub, "scale": scale, "shift": shift}


def exact_inputs(name, c):
    """the exact family's integers (module docstring), float32 arrays"""
    g = _gen("bf16exact" + c["mode"] + name)
    ints = lambda shape, lo, hi: torch.randint(lo, hi + 1, shape, generator=g).float().numpy()
    x = ints((c["b"], c["h"], c["w"], c["cin"]), -8, 8)
    wt = ints((9, c["cout"], c["cin"]), -8, 8)
    in_sub = ints((c["cin"],), -2, 2) if c["sub"] else None
    scale = (2.0 ** ints((c["cout"],), 0, 1)) * (2.0 * ints((c["cout"],), 0, 1) - 1.0) if c["affine"] else None
    shift = ints((c["cout"],), -8, 8) if c["affine"] else None
    return {"x": x, "wt": wt, "in_sub": in_sub, "scale": scale, "shift": shift}


def operands(x, wt, in_sub=None):
    """fp32 host tensors -> xb, wb: the bits the kernel forms, as fp32 tensors.  The subtraction is one fp32 operation"""
    xs = x if in_sub is None else x - in_sub          # fp32 - fp32, rounded once
    assert xs.dtype == torch.float32
    return bf16_round(xs), bf16_round(wt)


def reference(up, x, wt, in_sub=None, scale=None, shift=None, relu=False, device="cpu"):
    """fp32 tensors x (b,h,w,cin), wt (9,cout,cin), in_sub / scale / shift or None -> y, bound, S (b,h',w',cout) fp64 on `device`,
    by the formulas of the module docstring"""
    xb, wb = operands(x.cpu(), wt.cpu(), None if in_sub is None else in_sub.cpu())
    xb, wb = xb.double().to(device), wb.double().to(device)
    z, s = upconv_tap_sum(xb, wb, device=device) if up else conv_tap_sum(xb, wb, None, device=device)
    cin, cout = wt.shape[2], wt.shape[1]
    sc = torch.ones(cout, dtype=torch.float64, device=device) if scale is None else scale.double().to(device)
    sh = torch.zeros(cout, dtype=torch.float64, device=device) if shift is None else shift.double().to(device)
    y = z * sc + sh
    bound = sc.abs() * (9 * cin + 8) * U2 * s + 2 * U2 * ((sc * z).abs() + sh.abs()) + FLOOR
    return (y.clamp(min=0.0) if relu else y), bound, s


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32))


def case_reference(c, t, device="cpu"):
    """-> y (rows, cout), bound (rows, cout) fp64 in output pixel order, max S"""
    y, bound, s = reference(c["mode"] == "up", _t(t["x"]), _t(t["wt"]), _t(t["in_sub"]), _t(t["scale"]), _t(t["shift"]), c["relu"], device)
    return y.reshape(-1, c["cout"]), bound.reshape(-1, c["cout"]), float(s.max())


def exact_condition(smax, t):
    """every partial sum and the epilogue's result are integers below 2^24"""
    shift = 0.0 if t["shift"] is None else float(np.abs(t["shift"]).max())
    return 2 * smax + shift < 2 ** 24


@functools.lru_cache(maxsize=None)
def small_case(family, mode, name):
    """(case, inputs, y, bound, max S) of a case of the rounding or the exact family, computed once"""
    c = TABLES[family][mode][name]
    t = (round_inputs if family == "round" else exact_inputs)(name, c)
    return (c, t) + case_reference(c, t)


def emulate(c, t):
    """the kernel's arithmetic in torch on the host: bf16 operands, fp32 accumulation tap by tap, the two-step fp32 epilogue
    -> (rows, cout) fp32"""
    xb, wb = operands(_t(t["x"]), _t(t["wt"]), _t(t["in_sub"]))
    b, h, w, cin = xb.shape
    cout = wb.shape[1]
    if c["mode"] == "conv":
        pad = torch.zeros((b, h + 2, w + 2, cin))
        pad[:, 1:h + 1, 1:w + 1] = xb
        z = torch.zeros((b, h, w, cout))
        for ky in range(3):
            for kx in range(3):
                z = z + pad[:, ky:ky + h, kx:kx + w] @ wb[3 * ky + kx].T
    else:
        z = torch.zeros((b, 2 * h, 2 * w, cout))
        for ky in range(3):
            for kx in range(3):
                iy, ix = torch.arange(1 if ky == 0 else 0, h), torch.arange(1 if kx == 0 else 0, w)
                if len(iy) and len(ix):
                    z[:, (2 * iy - 1 + ky)[:, None], (2 * ix - 1 + kx)[None, :]] += xb[:, iy][:, :, ix] @ wb[3 * ky + kx].T
    if c["affine"]:
        z = z * _t(t["scale"])
        z = z + _t(t["shift"])
    return (z.clamp(min=0.0) if c["relu"] else z).reshape(-1, cout)


def abi_cases():
    """[{"id", "family", "kernels"}] of every C-ABI case of tests/test_conv_bf16_abi.py"""
    out = []
    for family, modes in TABLES.items():
        for mode, table in modes.items():
            for name, c in table.items():
                out.append({"id": "%s/%s/%s" % (mode, family, name), "family": family, "kernels": {instantiation(c)}})
    for name, c in REGIME_CASES.items():
        out.append({"id": "%s/regime/%s" % (c["mode"], name), "family": "regime", "kernels": {instantiation(c)}})
    return out


def selected_instantiations(cases=None):
    out = set()
    for c in (abi_cases() if cases is None else cases):
        out |= c["kernels"]
    return out


def einval_calls(L, one):
    """{what: status} of calls that must return HF_EINVAL before any HIP call (fake non-null pointers, never dereferenced)"""
    def conv(b=1, h=4, w=4, cin=8, cout=32, x=one, wt=one, y=one, stride=None, col=0):
        return L.hf_conv3x3_nhwc_bf16(b, h, w, cin, cout, x, None, wt, None, None, 1, y, cout if stride is None else stride, col, None)

    def up(b=1, h=4, w=4, cin=8, cout=32, x=one, wt=one, y=one, stride=None, col=0):
        return L.hf_upconv3x3s2_nhwc_bf16(b, h, w, cin, cout, x, wt, None, None, 1, y, cout if stride is None else stride, col, None)

    bad = {}
    for name, f in (("conv", conv), ("upconv", up)):
        bad.update({name + ": b = 0": f(b=0), name + ": h = 0": f(h=0), name + ": w = 0": f(w=0), name + ": cin = 0": f(cin=0),
                    name + ": cout = 0": f(cout=0), name + ": cout = 257": f(cout=257), name + ": y_col < 0": f(col=-1),
                    name + ": slice past the stride": f(stride=40, col=9), name + ": stride < cout": f(stride=31),
                    name + ": no x": f(x=None), name + ": no wt_bf16": f(wt=None), name + ": no y": f(y=None),
                    name + ": b negative": f(b=-1), name + ": b h w = 2^31": f(b=1 << 11, h=1 << 10, w=1 << 10)})
    bad["upconv: 4 b h w = 2^31"] = up(b=1 << 9, h=1 << 10, w=1 << 10)
    return bad


# ------------------------------------------------------------------------------------------------ the module, layer by layer
MODEL_CONV_DEEP = ((2, 8), (3, 16), (2, 16), (3, 32))      # two and three layers per block


def module_layers(net):
    """the module's layers in forward_native's launch order -> [(tap name, seq, source)], wired as image_pyramid_cases.module_forward
    wires them: source = "image" | a tap name (that output, dense) | ("cat", encoder tap, up tap): [encoder | up]"""
    recs, prev = [], "image"
    last = {}
    for level, block in enumerate((net.conv1, net.conv2, net.conv3, net.conv4)):
        for i, seq in enumerate(block):
            name = "conv%d_%d" % (level + 1, i)
            recs.append((name, seq, prev))
            prev = name
        last[level] = prev
        if level < 3:
            recs.append(("pool%d" % (level + 1), None, prev))
            prev = "pool%d" % (level + 1)
    for level, up, fusion in zip((2, 1, 0), (net.upconv3, net.upconv2, net.upconv1), (net.fusion3, net.fusion2, net.fusion1)):
        recs.append(("upconv%d" % (level + 1), up, prev))
        recs.append(("fusion%d" % (level + 1), fusion, ("cat", last[level], "upconv%d" % (level + 1))))
        prev = "fusion%d" % (level + 1)
    return recs


def layer_reference(seq, x, in_sub=None):
    """a _ConvBNReLU / _UpConvBNReLU of the host module and its input x (b,h,w,cin) fp32 -> y, bound fp64, from the module's own
    weights (tap t = 3 ky + kx) and its BatchNorm folded in fp64 and cast, as image_pyramid.fold_bn states it"""
    conv, bn = seq[0], seq[1]
    up = isinstance(conv, torch.nn.ConvTranspose2d)
    w = conv.weight.detach().cpu().float()
    wt = (w.permute(2, 3, 1, 0) if up else w.permute(2, 3, 0, 1)).reshape(9, w.shape[1] if up else w.shape[0], -1).contiguous()
    scale = bn.weight.detach().cpu().double() / torch.sqrt(bn.running_var.cpu().double() + bn.eps)
    shift = bn.bias.detach().cpu().double() - bn.running_mean.cpu().double() * scale
    y, bound, _ = reference(up, x.cpu(), wt, in_sub, scale.float(), shift.float(), True)
    return y, bound
