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

Next to that rounding family stands an exact one (integer-valued inputs: every partial sum is an fp32 number, the comparison is bit for
bit at any summation order), the launch-regime cases (exact inputs at production grid sizes, their fp64 tap sums formed on the device by
torch) and the dispatch rules of the launchers restated, so that tests/test_image_pyramid_instantiations_cpu.py can hold what the cases
select against what conv_nhwc.hip compiles to.

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
def conv_tap_sum(x, wt, in_sub=None, device=None):
    """x (b,h,w,cin), wt (9,cout,cin), fp64 tensors -> z, S (b,h,w,cout); device: where the sums are formed (default: where x is)"""
    device = x.device if device is None else device
    x, wt, in_sub = x.to(device), wt.to(device), None if in_sub is None else in_sub.to(device)
    b, h, w, cin = x.shape
    xs = x if in_sub is None else x - in_sub
    pad = torch.zeros((b, h + 2, w + 2, cin), dtype=torch.float64, device=device)
    pad[:, 1:h + 1, 1:w + 1] = xs                           # the padding stays zero: in_sub is not subtracted from it
    z = torch.zeros((b, h, w, wt.shape[1]), dtype=torch.float64, device=device)
    s = torch.zeros_like(z)
    for ky in range(3):
        for kx in range(3):
            src = pad[:, ky:ky + h, kx:kx + w]              # pixel (oy + ky - 1, ox + kx - 1)
            z += src @ wt[3 * ky + kx].T
            s += src.abs() @ wt[3 * ky + kx].abs().T
    return z, s


def upconv_tap_sum(x, wt, device=None):
    """x (b,h,w,cin), wt (9,cout,cin) -> z, S (b,2h,2w,cout): input pixel iy feeds output row 2 iy - 1 + ky"""
    device = x.device if device is None else device
    x, wt = x.to(device), wt.to(device)
    b, h, w, _ = x.shape
    z = torch.zeros((b, 2 * h, 2 * w, wt.shape[1]), dtype=torch.float64, device=device)
    s = torch.zeros_like(z)
    for ky in range(3):
        for kx in range(3):
            iy = torch.arange(1 if ky == 0 else 0, h, device=device)       # 2 iy - 1 + ky >= 0; it is <= 2 h - 1 for every iy
            ix = torch.arange(1 if kx == 0 else 0, w, device=device)
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


def conv_s2_tap_sum(x, wt, device=None):
    """x (b,2h,2w,cin), wt (9,cout,cin) fp64 -> z, S (b,h,w,cout): output (oy, ox) reads input (2 oy - 1 + ky, 2 ox - 1 + kx)"""
    device = x.device if device is None else device
    x, wt = x.to(device), wt.to(device)
    b, h2, w2, cin = x.shape
    pad = torch.zeros((b, h2 + 1, w2 + 1, cin), dtype=torch.float64, device=device)
    pad[:, 1:, 1:] = x
    z = torch.zeros((b, h2 // 2, w2 // 2, wt.shape[1]), dtype=torch.float64, device=device)
    s = torch.zeros_like(z)
    for ky in range(3):
        for kx in range(3):
            src = pad[:, ky:ky + h2:2, kx:kx + w2:2]                 # pad index 2 oy + ky = input index 2 oy - 1 + ky
            z += src @ wt[3 * ky + kx].T
            s += src.abs() @ wt[3 * ky + kx].abs().T
    return z, s


# ------------------------------------------------------------------------------------------------ the dispatch rules, restated
# Which kernel of conv_nhwc.hip a call launches and on what grid, restated from launch_conv, launch_conv_nt, hf_maxpool2x2_nhwc and
# hf_maxpool2x2_nhwc_bwd (conv_nhwc.hip), resident_grid and vec4_ok (gemm_common.h) and grid_for (hf_common.h); nothing is imported
# from the library.  tests/test_image_pyramid_cases_cpu.py looks the constants and the rule texts up in the sources,
# tests/test_image_pyramid_instantiations_cpu.py compares what the cases select with what the file compiles to.
NUM_CU = 256                    # hf_common.h kNumCU
BN_MAX_BLOCKS = 2048            # hf_common.h kBnMaxBlocks: the cap of resident_grid
FWD_ROWS = 128                  # gemm_common.h kFwdRows
FWD_KC = 32                     # gemm_common.h kFwdKC
GEMM_THREADS = 256              # gemm_common.h kGemmThreads
PER_CU = (5, 4, 3, 3, 2, 2, 2, 2)    # gemm_common.h resident_grid: per_cu[NT]
ROUNDS = 2                      # gemm_common.h resident_grid: the product build's constant
POOL_THREADS = 256              # conv_nhwc.hip: the block of the four pool launches
POOL_MAX_GRID = NUM_CU * 8      # hf_common.h grid_for: at most 8 workgroups per CU
CONV_MODES = ("conv", "up", "s2")    # conv_nhwc.hip kConvPlain, kConvUp, kConvS2 = 0, 1, 2
UP_CLASS_TAPS = (1, 2, 2, 4)    # conv_nhwc.hip: ntaps = (1 + py) (1 + px) of the four parity classes

SOURCE_CONSTANTS = (("hf_common.h", "kNumCU", NUM_CU), ("hf_common.h", "kBnMaxBlocks", BN_MAX_BLOCKS), ("gemm_common.h", "kFwdRows", FWD_ROWS),
                    ("gemm_common.h", "kFwdKC", FWD_KC), ("gemm_common.h", "kGemmThreads", GEMM_THREADS))
SOURCE_RULES = (
    ("conv_nhwc.hip", "constexpr int kConvPlain = 0, kConvUp = 1, kConvS2 = 2;"),
    ("conv_nhwc.hip", "const int ntaps = UP ? (1 + py) * (1 + px) : 9;"),
    ("conv_nhwc.hip", "if (cout <= 32) { HF_CONV_NT(1); }"),
    ("conv_nhwc.hip", "if (cout <= 64) { HF_CONV_NT(2); }"),
    ("conv_nhwc.hip", "if (cout <= 128) { HF_CONV_NT(4); }"),
    ("conv_nhwc.hip", "return vec4_ok(x, cin) && vec4_ok(wt, cin)"),
    ("conv_nhwc.hip", "const int ntiles = div_up(rows, kFwdRows);"),
    ("conv_nhwc.hip", "dim3(resident_grid(NT, ntiles), MODE == kConvUp ? 4 : 1)"),
    ("conv_nhwc.hip", "for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {"),
    ("conv_nhwc.hip", "(reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;"),
    ("conv_nhwc.hip", "const bool vec4 = c % 4 == 0 && x_stride % 4 == 0 && x_col % 4 == 0 && dx_stride % 4 == 0 && dx_col % 4 == 0 &&"),
    ("conv_nhwc.hip", "(reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dpooled)) % 16 == 0;"),
    ("conv_nhwc.hip", "const long long pixels = static_cast<long long>(b) * oh * ow;"),
    ("conv_nhwc.hip", "dim3(grid_for(pixels * (c / 4), 256)), dim3(256)"),
    ("conv_nhwc.hip", "dim3(grid_for(pixels * c, 256)), dim3(256)"),
    ("conv_nhwc.hip", "const int ch = (h + 1) / 2, cw = (w + 1) / 2;"),
    ("conv_nhwc.hip", "dim3(grid_for(cells * (c / 4), 256)), dim3(256)"),
    ("conv_nhwc.hip", "dim3(grid_for(cells * c, 256)), dim3(256)"),
    ("gemm_common.h", "static const int per_cu[9] = { 0, 5, 4, 3, 3, 2, 2, 2, 2 };"),
    ("gemm_common.h", "static const int rounds = HF_DIAG_INT(\"HF_GEMM_ROUNDS\", 2) < 1 ? 1 : HF_DIAG_INT(\"HF_GEMM_ROUNDS\", 2);"),
    ("gemm_common.h", "long long g = static_cast<long long>(kNumCU) * per_cu[nt < 1 ? 1 : (nt > 8 ? 8 : nt)] * rounds;"),
    ("gemm_common.h", "if (g > kBnMaxBlocks) g = kBnMaxBlocks;"),
    ("gemm_common.h", "inline bool vec4_ok(const void *p, int ncols) { return ncols % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0; }"),
    ("hf_common.h", "const long long cap = static_cast<long long>(kNumCU) * 8;"),
    ("hf_common.h", "#define HF_DIAG_INT(name, dflt) (dflt)"),
)


def cdiv(a, b):
    return (a + b - 1) // b


def conv_nt(cout):
    return 1 if cout <= 32 else 2 if cout <= 64 else 4 if cout <= 128 else 8


def conv_instantiation(case, off=None):
    """the kernel hf_conv3x3_nhwc (mode "conv"), hf_upconv3x3s2_nhwc ("up") or hf_conv3x3s2_nhwc ("s2") launches for the case;
    off: the operand ("x" or "wt") that sits one float past a 16-byte boundary"""
    vec = case["cin"] % 4 == 0 and off not in ("x", "wt")
    return ("conv3x3_kernel", (conv_nt(case["cout"]), vec, CONV_MODES.index(case.get("mode", "conv"))))


def resident_grid(nt, tiles):
    return min(NUM_CU * PER_CU[nt - 1] * ROUNDS, BN_MAX_BLOCKS, tiles)


def conv_rows(case):
    """the rows of the GEMM: the pixels of the grid the rows run over.  (b, h, w) of a case is that grid: the output of a plain or a
    stride-2 convolution, the INPUT of an up-convolution (every parity class, blockIdx.y, is a GEMM over the input pixels)"""
    return case["b"] * case["h"] * case["w"]


def conv_tiles(case):
    """(fewest, most) 128-row tiles a workgroup of the persistent grid walks: workgroup g owns tiles g, g + grid, g + 2 grid, ..."""
    tiles = cdiv(conv_rows(case), FWD_ROWS)
    grid = resident_grid(conv_nt(case["cout"]), tiles)
    return tiles // grid, cdiv(tiles, grid)


def conv_stages(case):
    """K stages of 32 per parity class (one entry for the plain and the stride-2 form): K = taps x cin"""
    taps = UP_CLASS_TAPS if case.get("mode", "conv") == "up" else (9,)
    return tuple(cdiv(t * case["cin"], FWD_KC) for t in taps)


def pool_slice(case, sliced):
    """(stride, col) of the pooled tensor's rows: a column slice of wider rows, or dense"""
    return (2 * case["c"] + 4, case["c"]) if sliced else (case["c"], 0)


def pool_instantiation(case, sliced, off=None, backward=False):
    """off: an operand one float past a 16-byte boundary.  The backward's dx has the stride and the column of x in every case"""
    stride, col = pool_slice(case, sliced)
    vec = 4 if case["c"] % 4 == 0 and stride % 4 == 0 and col % 4 == 0 and off is None else 1
    return ("maxpool2x2_bwd_kernel" if backward else "maxpool2x2_kernel", (vec,))


def pool_items(case, sliced=False, backward=False):
    """work items of a launch: output pixels (forward) or 2x2 cells, those of a last odd row or column included (backward), times
    c / VEC.  One lane takes an item, then strides by the grid"""
    vec = pool_instantiation(case, sliced, backward=backward)[1][0]
    cells = case["b"] * cdiv(case["h"], 2) * cdiv(case["w"], 2) if backward else case["b"] * (case["h"] // 2) * (case["w"] // 2)
    return cells * (case["c"] // vec)


def pool_strides(case, sliced=False, backward=False):
    """a lane takes more than one item: the grid is capped at POOL_MAX_GRID workgroups"""
    return pool_items(case, sliced, backward) > POOL_MAX_GRID * POOL_THREADS


# ------------------------------------------------------------------------------------------------ the exact family
# Inputs for which every partial sum of every kernel is an fp32 number: x integers in [-8, 8], in_sub integers in [-2, 2], wt sparse
# in {-1, 0, 1}, scale in {+-0.5, +-1, +-2}, shift multiples of 0.25 in [-4, 4].  |x'| <= 10 and at most 9 * 256 terms: every partial
# sum of z, in any order, chunking or tile walk, is an integer of magnitude <= S = sum |x'| |wt| <= 23040 < 2^24; y = z scale + shift is
# a multiple of 1/8 of magnitude <= 2 S + 4, an fp32 number while 8 (2 S + 4) < 2^24.  exact_condition gives S per case and the CPU
# test asserts 8 (2 S + 4) < 2^24.  A dropped product, a stale prefetch or a misindexed gather then changes bits at whatever order
# the sum is formed in: the comparison is abi_harness.same, no bound.
EXACT_COUT = (1, 32, 33, 64, 65, 128, 129, 256)          # both edges of every NT
EXACT_CIN = (3, 4, 5, 32, 33, 36, 256)                   # K = taps x cin staged 32 wide: 4 one stage and a 4-wide tail (one up tap); 5, 33
                                                         # a scalar quad over two taps; 32 whole stages; 36 a tail; 3 the first layer
EXACT_ALIGN_COUT = (32, 40, 128, 256)                    # one per NT, cin = 36 on (1, 12, 22): x, then wt, one float past the boundary


def _exact_case(mode, b, h, w, cin, cout, flags, off=None):
    sub, affine, relu, sl = flags
    c = dict(mode=mode, b=b, h=h, w=w, cin=cin, cout=cout, sub=bool(sub) and mode == "conv", affine=bool(affine), relu=bool(relu),
             slice=bool(sl), off=off)
    return "b%dh%dw%d_ci%d_co%d%s" % (b, h, w, cin, cout, "_off_" + off if off else ""), c


def exact_conv_cases(mode):
    """every (cin, cout) of EXACT_CIN x EXACT_COUT once; the geometry and the flags rotate so that every cin and every cout meet every
    geometry and every flag pattern; then the misaligned cases.  (b, h, w): see conv_rows"""
    cases = {}
    for i, cin in enumerate(EXACT_CIN):
        for j, cout in enumerate(EXACT_COUT):
            b, h, w = CONV_SHAPES[(i + j) % len(CONV_SHAPES)]
            name, c = _exact_case(mode, b, h, w, cin, cout, FLAG_PATTERNS[(len(EXACT_COUT) * i + j) % len(FLAG_PATTERNS)])
            cases[name] = c
    for j, cout in enumerate(EXACT_ALIGN_COUT):
        for k, off in enumerate(("x", "wt")):
            name, c = _exact_case(mode, 1, 12, 22, 36, cout, FLAG_PATTERNS[(2 * j + k) % len(FLAG_PATTERNS)], off)
            cases[name] = c
    return cases


EXACT_CONV_CASES = exact_conv_cases("conv")
EXACT_UPCONV_CASES = exact_conv_cases("up")
EXACT_S2_CASES = exact_conv_cases("s2")                  # run by tests/test_image_pyramid_train_abi.py, next to the rounding family's

# The launch regimes of production: a persistent grid whose every workgroup walks two tiles and some a third (the prefetch of the next
# tile's first stage under the MFMAs of the last stage), image rows and image boundaries inside tiles, a ragged last tile
REGIME_CONV_CASES = {
    "nt1_vec": dict(mode="conv", b=3, h=349, w=501, cin=4, cout=8, sub=True, affine=True, relu=True, slice=True, off=None),
    "first_layer": dict(mode="conv", b=3, h=349, w=501, cin=3, cout=32, sub=True, affine=True, relu=True, slice=False, off=None),
    "nt8_vec": dict(mode="conv", b=2, h=257, w=511, cin=4, cout=129, sub=False, affine=True, relu=False, slice=True, off=None),
}
REGIME_UPCONV_CASES = {"nt1_vec": dict(mode="up", b=3, h=349, w=501, cin=4, cout=8, sub=False, affine=True, relu=True, slice=True, off=None)}
REGIME_S2_CASES = {"nt1_vec": dict(mode="s2", b=3, h=349, w=501, cin=4, cout=8, sub=False, affine=True, relu=False, slice=True, off=None)}
# grid-stride pool launches: more items than POOL_MAX_GRID x POOL_THREADS lanes
REGIME_POOL_CASES = {"vec4": dict(b=1, h=514, w=516, c=32), "vec1": dict(b=1, h=838, w=837, c=3)}
REGIME_POOL_BWD_CASES = {"vec4": dict(b=1, h=513, w=515, c=32), "vec1": dict(b=1, h=837, w=835, c=3)}


def _exact_gen(name):
    return torch.Generator().manual_seed(zlib.crc32(("exact" + name).encode()))


def exact_conv_inputs(name, c):
    """float32 arrays of the exact family, seeded by mode and name: x, wt, in_sub / scale / shift or None"""
    import gemm_cases as gc
    g = _exact_gen(c["mode"] + name)
    k = 2 if c["mode"] == "s2" else 1
    x = gc.ints(g, (c["b"], k * c["h"], k * c["w"], c["cin"]), -8, 8).numpy()
    wt = gc.sparse_pm1(g, (9, c["cout"], c["cin"])).numpy()
    in_sub = gc.ints(g, (c["cin"],), -2, 2).numpy() if c["sub"] else None
    scale = (torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c["cout"],), generator=g)] * (2.0 * gc.ints(g, (c["cout"],), 0, 1) - 1.0)).numpy() \
        if c["affine"] else None
    shift = (gc.ints(g, (c["cout"],), -16, 16) / 4.0).numpy() if c["affine"] else None
    return {"x": x, "wt": wt, "in_sub": in_sub, "scale": scale, "shift": shift}


def exact_conv_reference(c, t, device="cpu"):
    """-> y (rows, cout) fp64 in output pixel order and max S, from the tap sums evaluated on `device`"""
    d = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64)).to(device)
    if c["mode"] == "conv":
        z, s = conv_tap_sum(d(t["x"]), d(t["wt"]), d(t["in_sub"]), device=device)
    else:
        z, s = (upconv_tap_sum if c["mode"] == "up" else conv_s2_tap_sum)(d(t["x"]), d(t["wt"]), device=device)
    smax = float(s.max())
    del s
    if c["affine"]:
        z = z * d(t["scale"]) + d(t["shift"])
    if c["relu"]:
        z = z.clamp(min=0.0)
    return z.reshape(-1, c["cout"]), smax


def exact_condition(smax):
    """every partial sum and the epilogue's result are fp32 numbers (the exact family's comment)"""
    return 8 * (2 * smax + 4) < 2 ** 24


@functools.lru_cache(maxsize=None)
def exact_conv_case(mode, name):
    """(case, inputs, y fp64 on the host, max S) of a small exact case, computed once"""
    c = {"conv": EXACT_CONV_CASES, "up": EXACT_UPCONV_CASES, "s2": EXACT_S2_CASES}[mode][name]
    t = exact_conv_inputs(name, c)
    y, smax = exact_conv_reference(c, t)
    return c, t, y, smax


def regime_pool_inputs(name, backward=False):
    """x ReLU-like on a grid of 0.5 (ties and all-zero windows); g and base small integers"""
    c = (REGIME_POOL_BWD_CASES if backward else REGIME_POOL_CASES)[name]
    rng = _rng("regimepool%d" % backward + name)
    x = np.maximum(np.round(rng.standard_normal((c["b"], c["h"], c["w"], c["c"]), dtype=np.float32) * 2.0) / 2.0, 0.0).astype(np.float32)
    g = rng.integers(-8, 9, (c["b"], c["h"] // 2, c["w"] // 2, c["c"])).astype(np.float32)
    base = rng.integers(-8, 9, x.shape).astype(np.float32)
    return {"x": x, "g": g, "base": base}


def abi_cases():
    """[{"id", "family" ("round", "exact" or "regime"), "kernels"}] of every C-ABI case of tests/test_image_pyramid_abi.py"""
    out = []
    add = lambda test, family, name, *kernels: out.append({"id": "%s/%s/%s" % (test, family, name), "family": family, "kernels": set(kernels)})
    for name, c in CONV_CASES.items():
        add("conv3x3", "round", name, conv_instantiation(c))
    add("conv3x3", "round", "b1h12w22_ci36_co40_off_x", conv_instantiation(CONV_CASES["b1h12w22_ci36_co40"], "x"))
    for name, c in UPCONV_CASES.items():
        add("upconv3x3s2", "round", name, conv_instantiation(dict(c, mode="up")))
    for test, family, table in (("conv3x3", "exact", EXACT_CONV_CASES), ("upconv3x3s2", "exact", EXACT_UPCONV_CASES),
                                ("conv3x3", "regime", REGIME_CONV_CASES), ("upconv3x3s2", "regime", REGIME_UPCONV_CASES)):
        for name, c in table.items():
            add(test, family, name, conv_instantiation(c, c["off"]))
    for family, table in (("round", POOL_CASES), ("regime", REGIME_POOL_CASES)):
        for name, c in table.items():
            add("maxpool2x2", family, name, pool_instantiation(c, True), pool_instantiation(c, False))
    return out


def selected_instantiations(cases=None):
    out = set()
    for c in (abi_cases() if cases is None else cases):
        out |= c["kernels"]
    return out


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
