"""Case tables, references and bounds of the image pyramid's training kernels (csrc/conv_nhwc.hip: hf_conv3x3_nhwc_wgrad,
hf_upconv3x3s2_nhwc_wgrad, hf_conv3x3s2_nhwc, hf_maxpool2x2_nhwc_bwd, and hf_conv3x3_nhwc used as an input gradient) and of
image_pyramid.forward_train.  tests/test_image_pyramid_train_cases_cpu.py checks this module on any machine,
tests/test_image_pyramid_train_abi.py runs the cases on the GPU through the C ABI, tests/test_image_pyramid_train.py goes through the
Python layer.  A plain helper module: the references come from the formulas of include/hfops.h, never from the kernels.

References, explicit fp64 sums in NHWC:
  wgrad            dwt[t][co][ci] = sum_p dz[p][co] x'[p + tap_t][ci], t = 3 ky + kx, x' = x - in_sub inside the image, zero in the padding
  up wgrad         dwt[t][co][ci] = sum_(iy,ix) dz[2 iy - 1 + ky, 2 ix - 1 + kx][co] x[iy, ix][ci] where that output pixel exists
  stride-2 conv    z[oy, ox, :] = sum_t x[2 oy - 1 + ky, 2 ox - 1 + kx, :] wt[t]^T, zero outside the image
  dgrad            conv_tap_sum of dz with w[t][ci][co] = wt[8 - t][co][ci]
  pool backward    torch's own CPU max_pool2d backward in fp32 (bit for bit); pool_bwd_rule restates its rule
Next to a weight gradient the reference forms S = sum |dz| |x'| over the same terms.

Bound of a weight-gradient element, derived (u = 2^-24): x - in_sub is rounded once (relative u, inside S to first order), every product is
formed exactly or with one rounding, and n = b h w terms are added in some order: |got - ref| <= (n + 2) u S + 2^-120 for ANY order.
The stride-2 convolution and the dgrad keep image_pyramid_cases.epilogue's bound, (9 cin + 2) u S and so on, cin being the channel
count that is summed over.

Inputs of a case are seeded by its name."""
import copy
import functools

import numpy as np
import torch
import torch.nn.functional as F

import image_pyramid_cases as pc
from image_pyramid_cases import FLOOR, U, _rng, _t64

# ------------------------------------------------------------------------------------------------ the tables
WGRAD_SHAPES = ((2, 5, 7), (1, 12, 22), (1, 40, 52), (3, 1, 1))   # 70 rows; 264: two chunks; 2080: several; one pixel: the centre tap only
WGRAD_CIN = (3, 36, 64, 256)
WGRAD_COUT = (32, 40, 256)
SUB_PATTERN = (1, 0, 1, 0, 0)                                      # in_sub on / off, five long: coprime to the 3 couts and the 4 cins


def _wgrad_cases():
    cases, i = {}, 0
    for b, h, w in WGRAD_SHAPES:
        for cin in WGRAD_CIN:
            for cout in WGRAD_COUT:
                cases["b%dh%dw%d_ci%d_co%d" % (b, h, w, cin, cout)] = dict(b=b, h=h, w=w, cin=cin, cout=cout,
                                                                            sub=bool(SUB_PATTERN[i % len(SUB_PATTERN)]))
                i += 1
    return cases


WGRAD_CASES = _wgrad_cases()
# (b, h, w) is the INPUT of the up-convolution; dz is (b, 2h, 2w, cout)
UPWGRAD_CASES = {"b%dh%dw%d_ci%d_co%d" % (b, h, w, cin, cout): dict(b=b, h=h, w=w, cin=cin, cout=cout, sub=False)
                 for b, h, w in ((2, 3, 5), (1, 1, 1), (1, 12, 22)) for cin in (36, 256) for cout in (32, 128)}
# (b, h, w) is the OUTPUT of the stride-2 convolution; x is (b, 2h, 2w, cin); always into a slice, every other case with the epilogue
S2_CASES = {"b%dh%dw%d_ci%d_co%d" % (b, h, w, cin, cout): dict(b=b, h=h, w=w, cin=cin, cout=cout, sub=False, slice=True,
                                                                affine=bool((s + i + j) % 2), relu=bool((s + i + j) % 2))
            for s, (b, h, w) in enumerate(((2, 3, 5), (1, 1, 1), (1, 6, 11))) for i, cin in enumerate((32, 128))
            for j, cout in enumerate((36, 256))}
# geometries of pc.CONV_CASES whose forward weights are flipped and transposed: the kernel then runs with cin and cout exchanged
DGRAD_CASES = ("b2h5w7_ci36_co40", "b1h12w22_ci64_co32", "b1h12w22_ci3_co32", "b3h1w1_ci256_co256", "b2h5w7_ci256_co32")
POOL_BWD_CASES = dict(pc.POOL_CASES)
POOL_NAN_CASE = "b2h6w10_c32"


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def wgrad_inputs(kind, name):
    """float32, read-only: x (b,h,w,cin), dz (b,h,w,cout) or (b,2h,2w,cout) for kind "up", in_sub (cin) or None"""
    c = (WGRAD_CASES if kind == "conv" else UPWGRAD_CASES)[name]
    rng = _rng("wgrad" + kind + name)
    k = 2 if kind == "up" else 1
    x = rng.uniform(-2.0, 2.0, (c["b"], c["h"], c["w"], c["cin"])).astype(np.float32)
    dz = rng.standard_normal((c["b"], k * c["h"], k * c["w"], c["cout"])).astype(np.float32)
    in_sub = rng.uniform(-1.0, 1.0, (c["cin"],)).astype(np.float32) if c["sub"] else None
    for a in (x, dz, in_sub):
        if a is not None:
            a.flags.writeable = False
    return {"x": x, "dz": dz, "in_sub": in_sub}


@functools.lru_cache(maxsize=None)
def s2_inputs(name):
    c = S2_CASES[name]
    rng = _rng("s2" + name)
    x = rng.uniform(-2.0, 2.0, (c["b"], 2 * c["h"], 2 * c["w"], c["cin"])).astype(np.float32)
    wt = (rng.standard_normal((9, c["cout"], c["cin"])) / np.sqrt(9.0 * c["cin"])).astype(np.float32)
    scale = (rng.uniform(0.5, 1.5, (c["cout"],)) * rng.choice([-1.0, 1.0], (c["cout"],))).astype(np.float32) if c["affine"] else None
    shift = rng.standard_normal((c["cout"],)).astype(np.float32) if c["affine"] else None
    for a in (x, wt, scale, shift):
        if a is not None:
            a.flags.writeable = False
    return {"x": x, "wt": wt, "scale": scale, "shift": shift}


@functools.lru_cache(maxsize=None)
def dgrad_inputs(name):
    """the forward case's weights and a gradient of its output: dz (b,h,w,cout), wt (9,cout,cin), wd (9,cin,cout) = flipped, transposed"""
    c = pc.CONV_CASES[name]
    wt = pc.conv_inputs("conv", name)["wt"]
    dz = _rng("dgrad" + name).standard_normal((c["b"], c["h"], c["w"], c["cout"])).astype(np.float32)
    wd = np.ascontiguousarray(wt[::-1].transpose(0, 2, 1))
    dz.flags.writeable = False
    wd.flags.writeable = False
    return {"dz": dz, "wt": wt, "wd": wd}


@functools.lru_cache(maxsize=None)
def pool_bwd_inputs(name):
    """x ReLU-like: about half exact zeros (all-zero windows tie), the positive values on a grid of 0.5 (duplicates inside windows);
    POOL_NAN_CASE has a NaN in two windows.  g: the gradient of the pooled output; base: what an accumulating call adds to"""
    c = POOL_BWD_CASES[name]
    rng = _rng("poolbwd" + name)
    x = np.maximum(np.round(rng.standard_normal((c["b"], c["h"], c["w"], c["c"])) * 2.0) / 2.0, 0.0).astype(np.float32)
    if name == POOL_NAN_CASE:
        x[0, 1, 1, 0] = np.nan
        x[1, 2, 3, 5] = np.nan
        x[1, 3, 3, 5] = np.nan                                    # two NaNs in one window: the later one wins
    g = rng.standard_normal((c["b"], c["h"] // 2, c["w"] // 2, c["c"])).astype(np.float32)
    base = rng.standard_normal(x.shape).astype(np.float32)
    for a in (x, g, base):
        a.flags.writeable = False
    return {"x": x, "g": g, "base": base}


# ------------------------------------------------------------------------------------------------ the sums
def conv_wgrad_sum(x, dz, in_sub=None):
    """x (b,h,w,cin), dz (b,h,w,cout) fp64 -> dwt, S (9,cout,cin)"""
    b, h, w, cin = x.shape
    pad = torch.zeros((b, h + 2, w + 2, cin), dtype=torch.float64)
    pad[:, 1:h + 1, 1:w + 1] = x if in_sub is None else x - in_sub
    g = dz.reshape(-1, dz.shape[-1])
    dwt = torch.zeros((9, dz.shape[-1], cin), dtype=torch.float64)
    s = torch.zeros_like(dwt)
    for ky in range(3):
        for kx in range(3):
            src = pad[:, ky:ky + h, kx:kx + w].reshape(-1, cin)      # x'[p + tap]
            dwt[3 * ky + kx] = g.T @ src
            s[3 * ky + kx] = g.abs().T @ src.abs()
    return dwt, s


def upconv_wgrad_sum(x, dz):
    """x (b,h,w,cin), dz (b,2h,2w,cout) fp64 -> dwt, S (9,cout,cin)"""
    b, h, w, cin = x.shape
    dwt = torch.zeros((9, dz.shape[-1], cin), dtype=torch.float64)
    s = torch.zeros_like(dwt)
    for ky in range(3):
        for kx in range(3):
            iy = torch.arange(1 if ky == 0 else 0, h)
            ix = torch.arange(1 if kx == 0 else 0, w)
            if not len(iy) or not len(ix):
                continue
            src = x[:, iy][:, :, ix].reshape(-1, cin)
            g = dz[:, 2 * iy - 1 + ky][:, :, 2 * ix - 1 + kx].reshape(-1, dz.shape[-1])
            dwt[3 * ky + kx] = g.T @ src
            s[3 * ky + kx] = g.abs().T @ src.abs()
    return dwt, s


def wgrad_bound(s, n):
    return (n + 2) * U * s + FLOOR


conv_s2_tap_sum = pc.conv_s2_tap_sum                                  # the forward kernel's third form: stated next to the other two


@functools.lru_cache(maxsize=None)
def wgrad_reference(kind, name):
    """-> {"dwt" (9,cout,cin) fp64, "bound"}"""
    c = (WGRAD_CASES if kind == "conv" else UPWGRAD_CASES)[name]
    t = wgrad_inputs(kind, name)
    dwt, s = conv_wgrad_sum(_t64(t["x"]), _t64(t["dz"]), _t64(t["in_sub"])) if kind == "conv" else upconv_wgrad_sum(_t64(t["x"]), _t64(t["dz"]))
    return {"dwt": dwt, "bound": wgrad_bound(s, c["b"] * c["h"] * c["w"])}


@functools.lru_cache(maxsize=None)
def s2_reference(name):
    c, t = S2_CASES[name], s2_inputs(name)
    z, s = conv_s2_tap_sum(_t64(t["x"]), _t64(t["wt"]))
    y, bound = pc.epilogue(z, s, c["cin"], _t64(t["scale"]), _t64(t["shift"]), c["relu"])
    return {"y": y.reshape(-1, c["cout"]), "bound": bound.reshape(-1, c["cout"])}


@functools.lru_cache(maxsize=None)
def dgrad_reference(name):
    """-> {"dx" (rows, cin) fp64, "bound"}: the sum runs over 9 cout terms, the existing bound with cin and cout exchanged"""
    c, t = pc.CONV_CASES[name], dgrad_inputs(name)
    z, s = pc.conv_tap_sum(_t64(t["dz"]), _t64(t["wd"]))
    y, bound = pc.epilogue(z, s, c["cout"])
    return {"dx": y.reshape(-1, c["cin"]), "bound": bound.reshape(-1, c["cin"])}


def pool_bwd_rule(x, g):
    """NumPy restatement of the rule: scan (0,0), (0,1), (1,0), (1,1); a strictly greater value or a NaN replaces the maximum"""
    b, h, w, c = x.shape
    dx = np.zeros_like(x)
    for oy in range(h // 2):
        for ox in range(w // 2):
            m = x[:, 2 * oy, 2 * ox].copy()
            k = np.zeros(m.shape, dtype=np.int64)
            for j, (dy, dx_) in enumerate(((0, 1), (1, 0), (1, 1)), start=1):
                v = x[:, 2 * oy + dy, 2 * ox + dx_]
                with np.errstate(invalid="ignore"):
                    take = (v > m) | np.isnan(v)
                m = np.where(take, v, m)
                k = np.where(take, j, k)
            for j, (dy, dx_) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                dx[:, 2 * oy + dy, 2 * ox + dx_] = np.where(k == j, g[:, oy, ox], 0.0)
    return dx


@functools.lru_cache(maxsize=None)
def pool_bwd_expected(name):
    """torch's CPU max_pool2d backward in fp32 -> {"grad" (b,h,w,c), "sum": base + grad, one fp32 add}"""
    t = pool_bwd_inputs(name)
    x = torch.from_numpy(t["x"].copy()).permute(0, 3, 1, 2).contiguous().requires_grad_()
    F.max_pool2d(x, 2).backward(torch.from_numpy(t["g"].copy()).permute(0, 3, 1, 2).contiguous())
    grad = x.grad.permute(0, 2, 3, 1).contiguous().numpy()
    return {"grad": grad, "sum": t["base"] + grad}


# ------------------------------------------------------------------------------------------------ the dispatch rules, restated
# launch_conv_wgrad and conv_wgrad_plan of conv_nhwc.hip, wgrad_plan of gemm_common.h (restated in gemm_cases.wgrad_plan); the pool's
# backward and the forward kernel's rules are image_pyramid_cases'.  tests/test_image_pyramid_train_cases_cpu.py looks the texts up.
SOURCE_RULES = (
    ("conv_nhwc.hip", "WgradPlan p = wgrad_plan(rows, 9 * cout, cin);"),
    ("conv_nhwc.hip", "if (p.wm != 2) { p.wm = 2; p.mtiles = 1; }      // 9 cout <= 64: one tile, partly empty"),
    ("conv_nhwc.hip", "using Q = WgradTile<2, WN>;"),
    ("conv_nhwc.hip", "const dim3 grid(p.mtiles * p.ntiles, p.chunks);"),
    ("conv_nhwc.hip", "const bool gvec = vec4_ok(dz, cout), xvec = vec4_ok(x, cin);"),
    ("conv_nhwc.hip", "if (p.wn == 2) HF_CWGRAD_V(2);"),
    ("conv_nhwc.hip", "return p.chunks > 1 ? sizeof(float) * static_cast<size_t>(p.chunks) * 9 * cout * cin : 0;"),
    ("gemm_common.h", "p.wm = cout > 64 ? 2 : 1;"),
    ("gemm_common.h", "p.wn = cin > 64 ? 2 : 1;"),
    ("gemm_common.h", "p.mtiles = div_up(cout, 64 * p.wm);"),
    ("gemm_common.h", "p.ntiles = div_up(cin, 64 * p.wn);"),
    ("gemm_common.h", "long long want = static_cast<long long>(kNumCU) * 3 / (p.mtiles * p.ntiles);"),
    ("gemm_common.h", "if (rpc < 256) rpc = 256;"),
)


def wgrad_instantiation(case, off=None):
    """the kernel hf_conv3x3_nhwc_wgrad or (case["up"]) hf_upconv3x3s2_nhwc_wgrad launches; off: "dz" or "x" one float past a
    16-byte boundary"""
    gvec = case["cout"] % 4 == 0 and off != "dz"
    xvec = case["cin"] % 4 == 0 and off != "x"
    return ("conv_wgrad_kernel", (2 if case["cin"] > 64 else 1, gvec, xvec, bool(case.get("up", False))))


def conv_wgrad_plan(case):
    """the plan of the (9 cout, cin) matrix over b h w reduction rows (for both directions the pixels of x), always with the 128-row
    M tile: {"wn", "mtiles", "ntiles", "rows_per_chunk", "chunks", "forced": 9 cout <= 64, one partly empty tile, "workspace": bytes}"""
    import gemm_cases as gc
    m, cin = 9 * case["cout"], case["cin"]
    wm, wn, rpc, chunks = gc.wgrad_plan(case["b"] * case["h"] * case["w"], m, cin)
    return {"wn": wn, "mtiles": 1 if wm != 2 else pc.cdiv(m, 128), "ntiles": pc.cdiv(cin, 64 * wn), "rows_per_chunk": rpc, "chunks": chunks,
            "forced": wm != 2, "workspace": 4 * chunks * m * cin if chunks > 1 else 0}


# ------------------------------------------------------------------------------------------------ the exact family
# image_pyramid_cases' family for the weight gradients: x integers in [-8, 8], in_sub in [-2, 2], dz sparse in {-1, 0, 1}: every
# partial sum of every chunk and of the reduction over chunks is an integer of magnitude <= S = sum |dz| |x'| <= 10 rows < 2^24
EXACT_WGRAD_COUT = (1, 7, 8, 5, 33, 32, 128)             # 9 cout <= 64 (1, 5, 7): the forced tile; 8 just past it; 5, 33: GVEC = false by shape
EXACT_WGRAD_CIN = (3, 5, 36, 64, 65, 68, 256)            # 64 | 65: WN; 65 is WN = 2 with a scalar X


def exact_wgrad_cases(up):
    """every (cin, cout) once, geometry and in_sub rotating; then dz and x, each in turn, one float past the boundary at both WN"""
    cases, n = {}, 0
    for i, cin in enumerate(EXACT_WGRAD_CIN):
        for j, cout in enumerate(EXACT_WGRAD_COUT):
            b, h, w = WGRAD_SHAPES[(i + j) % len(WGRAD_SHAPES)]
            cases["b%dh%dw%d_ci%d_co%d" % (b, h, w, cin, cout)] = dict(up=up, b=b, h=h, w=w, cin=cin, cout=cout, off=None,
                                                                        sub=bool(SUB_PATTERN[n % len(SUB_PATTERN)]) and not up)
            n += 1
    for cin, cout in ((36, 32), (68, 128)):
        for k, off in enumerate(("dz", "x")):
            cases["b1h12w22_ci%d_co%d_off_%s" % (cin, cout, off)] = dict(up=up, b=1, h=12, w=22, cin=cin, cout=cout, off=off,
                                                                          sub=k == 0 and not up)
    return cases


EXACT_WGRAD_CASES = exact_wgrad_cases(False)
EXACT_UPWGRAD_CASES = exact_wgrad_cases(True)            # (b, h, w) is the INPUT of the up-convolution
EXACT_S2_CASES, REGIME_S2_CASES = pc.EXACT_S2_CASES, pc.REGIME_S2_CASES


@functools.lru_cache(maxsize=None)
def exact_wgrad_case(up, name):
    """(case, inputs as float32 arrays, dwt (9,cout,cin) fp64, max S), computed once"""
    import gemm_cases as gc
    c = (EXACT_UPWGRAD_CASES if up else EXACT_WGRAD_CASES)[name]
    g = pc._exact_gen("wgrad%d" % up + name)
    k = 2 if up else 1
    t = {"x": gc.ints(g, (c["b"], c["h"], c["w"], c["cin"]), -8, 8).numpy(),
         "dz": gc.sparse_pm1(g, (c["b"], k * c["h"], k * c["w"], c["cout"])).numpy(),
         "in_sub": gc.ints(g, (c["cin"],), -2, 2).numpy() if c["sub"] else None}
    dwt, s = upconv_wgrad_sum(_t64(t["x"]), _t64(t["dz"])) if up else conv_wgrad_sum(_t64(t["x"]), _t64(t["dz"]), _t64(t["in_sub"]))
    return c, t, dwt, float(s.max())


def abi_cases():
    """[{"id", "family", "kernels"}] of every C-ABI case of tests/test_image_pyramid_train_abi.py (image_pyramid_cases.abi_cases'
    form); the dgrad cases run the forward kernel with cin and cout exchanged"""
    out = []
    add = lambda test, family, name, *kernels: out.append({"id": "%s/%s/%s" % (test, family, name), "family": family, "kernels": set(kernels)})
    for test, up, table in (("wgrad", False, WGRAD_CASES), ("upwgrad", True, UPWGRAD_CASES)):
        for name, c in table.items():
            add(test, "round", name, wgrad_instantiation(dict(c, up=up)))
    add("wgrad", "round", "b1h12w22_ci36_co40_off_x", wgrad_instantiation(WGRAD_CASES["b1h12w22_ci36_co40"], "x"))
    for test, table in (("wgrad", EXACT_WGRAD_CASES), ("upwgrad", EXACT_UPWGRAD_CASES)):
        for name, c in table.items():
            add(test, "exact", name, wgrad_instantiation(c, c["off"]))
    for name, c in S2_CASES.items():
        add("conv3x3s2", "round", name, pc.conv_instantiation(dict(c, mode="s2")))
    for family, table in (("exact", EXACT_S2_CASES), ("regime", REGIME_S2_CASES)):
        for name, c in table.items():
            add("conv3x3s2", family, name, pc.conv_instantiation(c, c["off"]))
    for name in DGRAD_CASES:
        c = pc.CONV_CASES[name]
        add("dgrad", "round", name, pc.conv_instantiation(dict(mode="conv", cin=c["cout"], cout=c["cin"])))
    for family, table in (("round", POOL_BWD_CASES), ("regime", pc.REGIME_POOL_BWD_CASES)):
        for name, c in table.items():
            add("maxpool2x2_bwd", family, name, pc.pool_instantiation(c, True, backward=True), pc.pool_instantiation(c, False, backward=True))
    return out


def selected_instantiations(cases=None):
    """what the cases of both ABI files reach in conv_nhwc.hip"""
    return pc.selected_instantiations(pc.abi_cases() + abi_cases() if cases is None else cases)


# ------------------------------------------------------------------------------------------------ HF_EINVAL
def einval_calls(L, one):
    """{what: status} of calls that must return HF_EINVAL before any HIP call (fake non-null pointers, never dereferenced)"""
    def s2(b=1, h=4, w=4, cin=8, cout=32, x=one, wt=one, y=one, stride=None, col=0):
        return L.hf_conv3x3s2_nhwc(b, h, w, cin, cout, x, wt, None, None, 1, y, cout if stride is None else stride, col, None)

    def wg(b=1, h=4, w=4, cin=8, cout=32, x=one, dz=one, dwt=one, ws=one, nbytes=1 << 40):
        return L.hf_conv3x3_nhwc_wgrad(b, h, w, cin, cout, x, None, dz, dwt, ws, nbytes, None)

    def uwg(b=1, h=4, w=4, cin=8, cout=32, x=one, dz=one, dwt=one, ws=one, nbytes=1 << 40):
        return L.hf_upconv3x3s2_nhwc_wgrad(b, h, w, cin, cout, x, dz, dwt, ws, nbytes, None)

    def pool(b=1, h=4, w=4, c=8, x=one, g=one, dx=one, xs=None, xc=0, ds=None, dc=0, acc=0):
        return L.hf_maxpool2x2_nhwc_bwd(b, h, w, c, x, c if xs is None else xs, xc, g, dx, c if ds is None else ds, dc, acc, None)

    bad = {}
    bad.update({"s2: b = 0": s2(b=0), "s2: h = 0": s2(h=0), "s2: w = 0": s2(w=0), "s2: cin = 0": s2(cin=0), "s2: cout = 0": s2(cout=0),
                "s2: cout = 257": s2(cout=257), "s2: y_col < 0": s2(col=-1), "s2: slice past the stride": s2(stride=40, col=9),
                "s2: stride < cout": s2(stride=31), "s2: no x": s2(x=None), "s2: no wt": s2(wt=None), "s2: no y": s2(y=None),
                "s2: b negative": s2(b=-1), "s2: b h w = 2^31": s2(b=1 << 11, h=1 << 10, w=1 << 10),
                "s2: 4 b h w = 2^31": s2(b=1 << 9, h=1 << 10, w=1 << 10)})
    for name, f in (("wgrad", wg), ("up wgrad", uwg)):
        bad.update({name + ": b = 0": f(b=0), name + ": h = 0": f(h=0), name + ": w = 0": f(w=0), name + ": cin = 0": f(cin=0),
                    name + ": cout = 0": f(cout=0), name + ": cout = 257": f(cout=257), name + ": cin = 513": f(cin=513),
                    name + ": no x": f(x=None), name + ": no dz": f(dz=None), name + ": no dwt": f(dwt=None), name + ": b negative": f(b=-1),
                    name + ": b h w = 2^31": f(b=1 << 11, h=1 << 10, w=1 << 10),
                    # 1 x 20 x 20 = 400 rows are two chunks: the partial matrices need a workspace
                    name + ": no workspace": f(h=20, w=20, ws=None), name + ": short workspace": f(h=20, w=20, nbytes=2 * 9 * 32 * 8 * 4 - 1)})
    bad["up wgrad: 4 b h w = 2^31"] = uwg(b=1 << 9, h=1 << 10, w=1 << 10)
    bad.update({"pool bwd: b = 0": pool(b=0), "pool bwd: h = 0": pool(h=0), "pool bwd: w = 0": pool(w=0), "pool bwd: c = 0": pool(c=0),
                "pool bwd: x_col < 0": pool(xc=-1), "pool bwd: x slice past the stride": pool(xs=12, xc=5),
                "pool bwd: dx_col < 0": pool(dc=-1), "pool bwd: dx slice past the stride": pool(ds=12, dc=5), "pool bwd: no x": pool(x=None),
                "pool bwd: no dpooled": pool(g=None), "pool bwd: no dx": pool(dx=None), "pool bwd: accumulate, no dx": pool(dx=None, acc=1)})
    return bad


def workspace_queries(L):
    """{what: bytes} of workspace queries that must return 0: outside the contract, or a single chunk"""
    out = {}
    for name, f in (("wgrad", L.hf_conv3x3_nhwc_wgrad_workspace), ("up wgrad", L.hf_upconv3x3s2_nhwc_wgrad_workspace)):
        out.update({name + ": b = 0": f(0, 4, 4, 8, 32), name + ": cout = 257": f(1, 4, 4, 8, 257), name + ": cin = 513": f(1, 4, 4, 513, 32),
                    name + ": h negative": f(1, -4, 4, 8, 32), name + ": b h w = 2^31": f(1 << 11, 1 << 10, 1 << 10, 8, 32),
                    name + ": a single chunk": f(2, 5, 7, 8, 32)})
    return out


# ------------------------------------------------------------------------------------------------ the module
TRAIN_SEED = 10              # the first seed of range(64) for which train_conditions holds (searched on the host: find_seed)
TRAIN_IMAGE = pc.MODEL_IMAGE


def make_train_model(seed=TRAIN_SEED):
    return pc.make_model(seed).train()


def make_cotangent(seed=TRAIN_SEED, net=None):
    shape = TRAIN_IMAGE[:3] + (pc.MODEL_CONV[0][1],)
    return torch.empty(shape).normal_(0.0, 1.0, generator=torch.Generator().manual_seed(2000 + seed))


def layer_sequences(net):
    """the sixteen-layer order of image_pyramid._train_layers, restated: [(name, Sequential)]"""
    out = []
    for block in ("conv1", "conv2", "conv3", "conv4"):
        out += [("%s.%d" % (block, i), seq) for i, seq in enumerate(getattr(net, block))]
    for name in ("upconv3", "fusion3", "upconv2", "fusion2", "upconv1", "fusion1"):
        out.append((name, getattr(net, name)))
    return out


def train_forward(net, image, detach=None, taps=None):
    """ImgVggPyr.forward restated for the training checks.  detach = ("skip", level): the encoder half of that level's concat is
    detached; ("pool", level): the pooled path below that level is.  taps: a dict that receives every pre-ReLU activation (the
    BatchNorm output) and every pool input, by name"""
    from heterofusionrcnn_amd.inference import IMAGE_MEAN
    x = image.permute(0, 3, 1, 2) - torch.tensor(IMAGE_MEAN, dtype=image.dtype).view(1, 3, 1, 1)

    def run(name, seq, x):
        for i, layer in enumerate(seq) if isinstance(seq[0], torch.nn.Sequential) else [(None, seq)]:
            pre = layer[1](layer[0](x))
            if taps is not None:
                taps["pre.%s" % (name if i is None else "%s.%d" % (name, i))] = pre.detach().clone()
            x = torch.relu(pre)
        return x

    def pool(level, enc):
        if taps is not None:
            taps["pool.%d" % level] = enc.detach().clone()
        p = F.max_pool2d(enc, 2)
        return p.detach() if detach == ("pool", level) else p

    skip = lambda level, enc: enc.detach() if detach == ("skip", level) else enc
    conv1 = run("conv1", net.conv1, x)
    conv2 = run("conv2", net.conv2, pool(1, conv1))
    conv3 = run("conv3", net.conv3, pool(2, conv2))
    conv4 = run("conv4", net.conv4, pool(3, conv3))
    f3 = run("fusion3", net.fusion3, torch.cat([skip(3, conv3), run("upconv3", net.upconv3, conv4)], dim=1))
    f2 = run("fusion2", net.fusion2, torch.cat([skip(2, conv2), run("upconv2", net.upconv2, f3)], dim=1))
    f1 = run("fusion1", net.fusion1, torch.cat([skip(1, conv1), run("upconv1", net.upconv1, f2)], dim=1))
    return f1.permute(0, 2, 3, 1).contiguous()


def _step(net, image, cot, forward=None, **kw):
    """one training forward and backward on the host -> {"out", "grad.<parameter>", "buf.<running statistic>"}, detached"""
    net.zero_grad(set_to_none=True)
    out = net(image) if forward is None else forward(net, image, **kw)
    out.backward(cot)
    res = {"out": out.detach()}
    res.update({"grad." + n: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for n, p in net.named_parameters()})
    res.update({"buf." + n: b.detach().clone() for n, b in net.named_buffers() if not n.endswith("num_batches_tracked")})
    return res


@functools.lru_cache(maxsize=None)
def train_reference(seed=TRAIN_SEED):
    """-> {"ref64": the fp64 module's output, gradients and updated running statistics, "tol": per tensor TOL_MARGIN max|fp32 host
    torch route - fp64|, "moves": {detach: the largest ratio |detached - ref64| / tolerance over the gradient tensors}, "margin":
    the mask conditions (see train_conditions)}; computed once per session"""
    net32, image, cot = make_train_model(seed), pc.make_image(seed, TRAIN_IMAGE), make_cotangent(seed)
    start = copy.deepcopy(net32.state_dict())
    fresh64 = lambda: copy.deepcopy(net32).double()
    net64 = fresh64()
    got32 = None
    ref64 = _step(net64, image.double(), cot.double())
    net32b = copy.deepcopy(net32)
    got32 = _step(net32b, image, cot)
    tol = {k: pc.TOL_MARGIN * float((got32[k].double() - ref64[k]).abs().max()) for k in ref64}
    # the restatement with taps, fp64 and fp32: it must be the module, and it gives the activations the masks depend on
    taps64, taps32 = {}, {}
    restated = _step(fresh64(), image.double(), cot.double(), train_forward, taps=taps64)
    assert all(torch.equal(restated[k], ref64[k]) for k in ref64), "train_forward does not restate ImgVggPyr.forward"
    _step(copy.deepcopy(net32), image, cot, train_forward, taps=taps32)
    moves = {}
    for level in (1, 2, 3):
        for what in ("skip", "pool"):
            r = _step(fresh64(), image.double(), cot.double(), train_forward, detach=(what, level))
            moves[(what, level)] = max(float((r[k] - ref64[k]).abs().max()) / tol[k] if tol[k] > 0 else 0.0
                                       for k in ref64 if k.startswith("grad."))
    # mask ambiguity: per activation its own forward tolerance (TOL_MARGIN x the fp32 route's error on that tensor)
    relu_margin, pool_margin = float("inf"), float("inf")
    for k, a64 in taps64.items():
        t = pc.TOL_MARGIN * float((taps32[k].double() - a64).abs().max())
        if k.startswith("pre."):
            relu_margin = min(relu_margin, float(a64.abs().min()) / t if t > 0 else float("inf"))
        else:
            b, c, h, w = a64.shape
            win = a64[:, :, :h // 2 * 2, :w // 2 * 2].reshape(b, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, c, h // 2, w // 2, 4)
            top = win.sort(dim=-1, descending=True).values
            gap = (top[..., 0] - top[..., 1])[~((top[..., 0] == 0) & (top[..., 1] == 0))]
            if gap.numel():
                pool_margin = min(pool_margin, float(gap.min()) / t if t > 0 else float("inf"))
    assert sorted(net32.state_dict()) == sorted(start)
    return {"ref64": ref64, "tol": tol, "fp32": got32, "moves": moves, "relu_margin": relu_margin, "pool_margin": pool_margin,
            "tracked": {n: int(b) for n, b in net64.named_buffers() if n.endswith("num_batches_tracked")}}


def train_conditions(r):
    """the three conditions that make the tolerances meaningful -> {name: bool}"""
    return {"every tolerance is above zero": all(t > 0 for t in r["tol"].values()),
            "every detached path moves a gradient by more than SWAP_FACTOR tolerances": all(m > pc.SWAP_FACTOR for m in r["moves"].values()),
            "no pre-ReLU activation within its tolerance of zero": r["relu_margin"] > 1.0,
            "no pool window whose two largest entries are within the tolerance": r["pool_margin"] > 1.0}


def find_seed(limit=64):
    for seed in range(limit):
        r = train_reference(seed)
        if all(train_conditions(r).values()):
            return seed
    return None
