"""Case table, inputs, fp64 references and derived bounds of the bf16 inference GEMM (csrc/linear_bf16.hip) -- shared by
tests/test_linear_bf16_abi.py (on the GPU, through the C ABI) and tests/test_linear_bf16_cpu.py (the coverage guard, on any machine).

Dispatch, restated from hf_linear_bf16_fwd_eval: a workgroup owns ROW_TILE = 128 rows and a column tile of
64 (cout <= 64: linear_bf16_kernel<2, 2>), 128 (cout <= 128: <4, 2>) or 256 columns (beyond: <4, 4>, eight waves); a K stage is 64
channels, cin % 4 == 0 and cout % 4 == 0.  The cases therefore add, to the sizes the families are asked to cover, rows one below, at and
one above ROW_TILE and the multiples of four next to and at every column tile (60 / 64 / 68, 124 / 128 / 132, 252 / 256 / 260).

EXACT  x, w integers in [-8, 8] (exact in bf16: 4 significant bits), every product an integer and every partial sum at most
       64 cin <= 81920 < 2^24: the fp32 accumulators hold the exact sum whatever the order inside and between MFMAs.  bias, mean in
       [-2, 2], gamma * invstd in {+-2, +-4}, beta odd: z + bias, z - mean, the product (below 2^20) and the sum are exact integers and
       the ReLU pre-activation is odd, hence nonzero.  The result equals the fp64 reference bit for bit.  ELU is off.
ROUND  seeded normal inputs.  Reference: fp64 on the operands rounded to bf16 by torch's CPU conversion (xb, wb).  With u' = 2^-23
       (twice the unit roundoff, so that an accumulator that truncates is still inside):
         z   products of two bf16 are exact in fp32; cin - 1 additions in some order, one for the bias:
             E_z = (cin + 8) u' (|xb| |wb|^T + |bias|)
         e   = elu(z) where mode & 2.  elu is 1-Lipschitz and continuous, the helper's stated error is ELU_C u (exp(z) + 1) <= 2 ELU_C u
             for z <= 0 (tests/bn_cases.py, measured there; u = 2^-24) and 0 for z > 0; the computed z may be non-positive wherever
             z_ref - E_z <= 0:   E_e = E_z + [z_ref - E_z <= 0] 2 ELU_C u
         y   = fl(fl(a fl(e - mean)) + beta), a = fl(gamma invstd): four roundings on top of the error of e.  With A = gamma invstd exact,
             |y - y_ref| <= |A| E_e + (4 u + O(u^2)) |A| (|e_ref - mean| + E_e) + u |beta|
                         <= |A| E_e + 3 u' (|A| (|e_ref - mean| + E_e) + |beta|) = E_y
         ReLU is 1-Lipschitz: E_y carries over.  The pre-activations are nevertheless kept RELU_MARGIN = 1e-3 from zero (rows with an
         element inside the margin get one input moved, before the call; asserted on the reference), so that no element is excused.
         With ELU and ReLU together a column's pre-activation tends to a (-1 - mean) + beta for very negative z whatever x is: beta is
         moved by 0.1 where that limit lies within 0.05 of zero.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_cases import ELU_C  # noqa: E402

U = 2.0 ** -24
U2 = 2.0 ** -23
RELU_MARGIN = 1e-3
ROW_TILE = 128
COL_TILES = (64, 128, 256)
K_STAGE = 64
CU_RESIDENT_WORKGROUPS = 256 * 3      # <2, 2>: 152 VGPRs -> three waves per SIMD, 30 KB of LDS: three workgroups per CU

# name -> (bn given, mode, bias)
MODES = {
    "plain": (False, 0, True),
    "plain_nobias": (False, 0, False),
    "bn": (True, 0, False),
    "bn_relu": (True, 1, True),
    "bn_elu": (True, 2, False),
    "bn_elu_relu": (True, 3, True),
}
EXACT_MODES = ("plain", "bn", "bn_relu")
ROUND_MODES = ("plain", "bn", "bn_relu", "bn_elu", "bn_elu_relu")


def column_tile(cout):
    return 64 if cout <= 64 else (128 if cout <= 128 else 256)


def instantiation(cout):
    return ("linear_bf16_kernel", {64: (2, 2), 128: (4, 2), 256: (4, 4)}[column_tile(cout)])


def workgroups(rows, cout):
    return -(-rows // ROW_TILE) * -(-cout // column_tile(cout))


def _case(family, rows, cin, cout, mode):
    return dict(family=family, rows=rows, cin=cin, cout=cout, mode=mode)


def case_id(c):
    return "%s-%dx%dx%d-%s" % (c["family"], c["rows"], c["cin"], c["cout"], c["mode"])


def exact_cases():
    out = []
    for rows in (1, 63, 64, 65, 257, 1000):
        for cin, cout in ((4, 4), (28, 36), (32, 128), (36, 132), (260, 228), (1280, 516)):
            for mode in EXACT_MODES:
                out.append(_case("exact", rows, cin, cout, mode))
    for rows in (ROW_TILE - 1, ROW_TILE, ROW_TILE + 1):
        out.append(_case("exact", rows, 36, 132, "bn_relu"))
    for cout in (60, 64, 68, 124, 128, 132, 252, 256, 260):
        out.append(_case("exact", 65, 68, cout, "bn_relu"))
    out.append(_case("exact", 131073, 64, 64, "bn_relu"))     # 1025 workgroups: more than the chip holds, and a grid that is no multiple of 8
    out.append(_case("exact", 257, 64, 516, "plain_nobias"))  # three column tiles per row block, cin exactly one stage
    return out


def round_cases():
    return [_case("round", rows, cin, cout, mode) for rows, cin, cout in ((1000, 260, 228), (257, 1280, 516), (65, 2688, 512))
            for mode in ROUND_MODES]


def all_cases():
    return exact_cases() + round_cases()


def selected_instantiations(cases=None):
    """the kernels the cases reach, by the dispatch rule above; the conversion kernel is reached by the known-answer test and by
    nothing else in the table"""
    return {instantiation(c["cout"]) for c in (all_cases() if cases is None else cases)} | {("f32_to_bf16_kernel", ())}


def generator(c):
    modes = sorted(MODES)
    return torch.Generator().manual_seed(((c["rows"] * 4099 + c["cin"]) * 4099 + c["cout"]) * 8 + modes.index(c["mode"]))


def bf16_round(t):
    """torch's CPU conversion (round to nearest even), back in fp32"""
    return t.cpu().to(torch.bfloat16).float()


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pick(g, shape, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]


def inputs(c):
    """host tensors: x, w (fp32; w is handed to the kernel through hf_f32_to_bf16), bias, bn = (gamma, beta, mean, invstd) or None"""
    g = generator(c)
    rows, cin, cout = c["rows"], c["cin"], c["cout"]
    has_bn, mode, has_bias = MODES[c["mode"]]
    if c["family"] == "exact":
        assert not mode & 2
        x, w = _ints(g, (rows, cin), -8, 8), _ints(g, (cout, cin), -8, 8)
        bias = _ints(g, (cout,), -2, 2) if has_bias else None
        bn = None
        if has_bn:      # gamma * invstd in {+-2, +-4}, beta odd: an odd pre-activation
            bn = (_pick(g, (cout,), [1.0, -1.0, 2.0, -2.0]), _pick(g, (cout,), [-3.0, -1.0, 1.0, 3.0]), _ints(g, (cout,), -2, 2),
                  _pick(g, (cout,), [2.0]))
    else:
        x, w = torch.randn(rows, cin, generator=g) + 0.3, torch.randn(cout, cin, generator=g) * 0.5
        bias = torch.randn(cout, generator=g) if has_bias else None
        bn = None
        if has_bn:
            bn = (torch.randn(cout, generator=g) * 0.5 + 1.0, torch.randn(cout, generator=g), torch.randn(cout, generator=g),
                  torch.rand(cout, generator=g) * 0.2 + 0.05)
        if mode == 3:   # elu saturates at -1: a column whose saturated pre-activation a (-1 - mean) + beta sits at zero cannot be moved by x
            gamma, beta, mean, invstd = bn
            sat = gamma * invstd * (-1.0 - mean) + beta
            bn = (gamma, torch.where(sat.abs() < 0.05, beta + 0.1, beta), mean, invstd)
        if mode & 1:
            x = nudge_rows_off_relu_threshold(x, w, bias, bn, mode)
    return dict(x=x, w=w, bias=bias, bn=bn)


def elu64(z):
    return torch.where(z > 0, z, torch.expm1(z.clamp(max=0)))


def reference(t, mode):
    """fp64 on the bf16-rounded operands -> dict(y, err, pre): err by the derivation in the module docstring, pre = the value the ReLU
    sees (None without ReLU)"""
    xb, wb = bf16_round(t["x"]).double(), bf16_round(t["w"]).double()
    cin = xb.shape[1]
    bias = t["bias"].double() if t["bias"] is not None else torch.zeros(wb.shape[0], dtype=torch.float64)
    z = xb @ wb.t() + bias
    e_z = (cin + 8) * U2 * (xb.abs() @ wb.abs().t() + bias.abs())
    if t["bn"] is None:
        return dict(y=z, err=e_z, pre=None)
    gamma, beta, mean, invstd = [v.double() for v in t["bn"]]
    e, e_e = z, e_z
    if mode & 2:
        e = elu64(z)
        e_e = e_z + (z - e_z <= 0).double() * 2 * ELU_C * U
    a = gamma * invstd
    pre = a * (e - mean) + beta
    err = a.abs() * e_e + 3 * U2 * (a.abs() * ((e - mean).abs() + e_e) + beta.abs())
    return dict(y=pre.clamp(min=0) if mode & 1 else pre, err=err, pre=pre if mode & 1 else None)


def nudge_rows_off_relu_threshold(x, w, bias, bn, mode):
    """rows with a ReLU pre-activation inside RELU_MARGIN get one input moved by a quarter until
    none is left (a wide layer has such an element in a good share of its rows: each pass clears most of them)"""
    x = x.clone()
    for it in range(32):
        pre = reference(dict(x=x, w=w, bias=bias, bn=bn), mode)["pre"]
        bad = (pre.abs() < 2 * RELU_MARGIN).any(dim=1)
        if not bool(bad.any()):
            return x
        x[bad, it % x.shape[1]] += 0.25
    raise AssertionError("ReLU pre-activations still inside the margin")


# ---- conversion known-answer values: where truncation and round-to-nearest-even differ, the ties, the overflow edge
def conversion_values():
    import struct
    f = lambda bits: struct.unpack("<f", struct.pack("<I", bits))[0]
    vals = [1.0 + 2.0 ** -8 + 2.0 ** -9,          # above the tie: up (truncation: down)
            1.0 + 2.0 ** -8,                      # tie, even below: down to 1
            1.0 + 3 * 2.0 ** -8,                  # tie, even above: up to 1 + 2^-6
            1.0 + 2.0 ** -9,                      # below the tie: down
            0.0, -0.0, 1.0, 3.140625,
            f(0x7F7F7FFF),                        # the largest value that stays finite
            f(0x7F7F8000),                        # the tie at the top: to even = Inf
            f(0x7F7FFFFF),                        # the largest finite fp32: Inf
            float("inf")]
    vals += [-v for v in vals if v != 0.0]
    return torch.tensor(vals, dtype=torch.float32)
