"""Case table, inputs, fp64 references and bounds of the bf16 training kernels (csrc/linear_bf16_train.hip) -- shared by
tests/test_linear_bf16_train_abi.py (on the GPU, through the C ABI) and tests/test_linear_bf16_train_cpu.py (the coverage guard, on
any machine).

Dispatch, restated from hf_linear_bf16_wgrad: dW (cout, cin) is cut into tiles of OUT_TILE = 128 outputs by 128 inputs
(cin <= 128: wgrad_bf16_kernel<2>) or 256 inputs (beyond: wgrad_bf16_kernel<4>, eight waves).  The rows are cut into chunks: about
3 * 256 workgroups are wanted in all, a chunk is the rows divided by the chunks wanted per tile, rounded up to the STAGE of 64 rows
(two K_STEPs of 32), and at least MIN_CHUNK = 256 rows.  One chunk writes dW directly; more go through the workspace and the
fixed-order reduction of hf_linear_wgrad (16 groups of chunks, four chunks in flight per group: more than 64 chunks reach its
unrolled loop).  The transposing conversion works on TR_TILE = 32 x 32 tiles.

EXACT  g, x integers in [-8, 8] (exact in bf16), every product an integer of at most 64 and 64 rows < 2^24: every partial sum, inside
       a chunk and between chunks, is exact in fp32 and the result equals fp64 bit for bit whatever the order.
ROUND  seeded normal inputs against fp64 on the operands rounded by torch's CPU bf16 conversion (g_b, x_b).  Products of two bf16 are
       exact in fp32; rows - 1 fp32 additions in any order stay within gamma_{rows - 1} of the absolute sum, and u' = 2^-23 (twice the
       unit roundoff) leaves room for an accumulator that truncates:  E = (rows + 8) u' |g_b|^T |x_b|.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_cases as lc  # noqa: E402
from linear_bf16_cases import U2, bf16_round  # noqa: E402,F401

OUT_TILE = 128
IN_TILES = (128, 256)
K_STEP = 32
STAGE = 64
MIN_CHUNK = 256
NUM_CU = 256
WANTED_WORKGROUPS = 3 * NUM_CU
REDUCE_UNROLLED_FROM = 65           # chunks: 16 groups x 4 in flight
TR_TILE = 32
# wgrad_bf16_kernel<2> (amdgpu_waves_per_eu(2), four waves): at most two workgroups per CU
CU_RESIDENT_WORKGROUPS = NUM_CU * 2


def in_tile(cin):
    return 128 if cin <= 128 else 256


def instantiation(cin):
    return ("wgrad_bf16_kernel", ({128: 2, 256: 4}[in_tile(cin)],))


def plan(rows, cout, cin):
    """(tiles, rows per chunk, chunks)"""
    tiles = -(-cout // OUT_TILE) * -(-cin // in_tile(cin))
    want = max(1, WANTED_WORKGROUPS // tiles)
    rpc = -(-rows // want)
    rpc = max(MIN_CHUNK, -(-rpc // STAGE) * STAGE)
    return tiles, rpc, -(-rows // rpc)


def workgroups(rows, cout, cin):
    tiles, _, chunks = plan(rows, cout, cin)
    return tiles * chunks


def _case(family, rows, cout, cin):
    return dict(family=family, rows=rows, cout=cout, cin=cin)


def case_id(c):
    return "%s-%dx%dx%d" % (c["family"], c["rows"], c["cout"], c["cin"])


def exact_cases():
    out = []
    for rows in (1, K_STEP - 1, K_STEP, K_STEP + 1, STAGE - 1, STAGE, STAGE + 1, MIN_CHUNK - 1, MIN_CHUNK, MIN_CHUNK + 1):
        for cout, cin in ((4, 4), (132, 36), (36, 260)):
            out.append(_case("exact", rows, cout, cin))
    for cout in (OUT_TILE - 4, OUT_TILE, OUT_TILE + 4):
        out.append(_case("exact", 300, cout, 68))
    for tile in IN_TILES:
        for cin in (tile - 4, tile, tile + 4):
            out.append(_case("exact", 300, 68, cin))
    out.append(_case("exact", 1000, 260, 260))      # six tiles, four chunks
    out.append(_case("exact", 17920, 64, 64))       # 70 chunks: the unrolled loop of the reduction and its tail
    out.append(_case("exact", 200000, 64, 64))      # 625 workgroups: more than the chip holds, and a grid that is no multiple of 8
    return out


def round_cases():
    return [_case("round", 300, 128, 128), _case("round", 1000, 64, 260), _case("round", 3000, 260, 64)]


def all_cases():
    return exact_cases() + round_cases()


def selected_instantiations(cases=None):
    """the kernels the cases reach, by the dispatch rule above; the transposing conversion is reached by transpose_cases() and the
    known-answer test"""
    return {instantiation(c["cin"]) for c in (all_cases() if cases is None else cases)} | {("f32_to_bf16_transpose_kernel", ())}


def generator(c):
    return torch.Generator().manual_seed((c["rows"] * 4099 + c["cout"]) * 4099 + c["cin"])


def inputs(c):
    """host tensors g (rows, cout), x (rows, cin)"""
    gen = generator(c)
    rows, cout, cin = c["rows"], c["cout"], c["cin"]
    if c["family"] == "exact":
        return dict(g=torch.randint(-8, 9, (rows, cout), generator=gen).float(), x=torch.randint(-8, 9, (rows, cin), generator=gen).float())
    return dict(g=torch.randn(rows, cout, generator=gen) * 0.5, x=torch.randn(rows, cin, generator=gen) + 0.3)


def reference(t):
    """fp64 on the bf16-rounded operands -> dict(dw, err)"""
    gb, xb = bf16_round(t["g"]).double(), bf16_round(t["x"]).double()
    rows = gb.shape[0]
    return dict(dw=gb.t() @ xb, err=(rows + 8) * U2 * (gb.abs().t() @ xb.abs()))


# ---- the transposing conversion: (rows, cols) of src
def transpose_cases():
    return [(4, 4), (1, 37), (37, 1), (TR_TILE, TR_TILE), (2 * TR_TILE, 3 * TR_TILE), (TR_TILE + 1, 2 * TR_TILE + 1), (100, 260), (516, 68)]


def transpose_input(rows, cols):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows * 4099 + cols)) * 3.0


def transpose_reference_bits(src):
    """torch's CPU conversion of the transposed tensor, as int16 bits"""
    return src.t().contiguous().to(torch.bfloat16).view(torch.int16)


def conversion_matrix():
    """the known-answer values of linear_bf16_cases.conversion_values() in column 1 of an otherwise random matrix"""
    vals = lc.conversion_values()
    m = transpose_input(vals.numel(), 5)
    m[:, 1] = vals
    return m


# ---- the input gradient as a composition: (rows, cout, cin), g (rows, cout) and W (cout, cin) integers
def dx_cases():
    return [(65, 36, 132), (300, 132, 260)]


def dx_inputs(rows, cout, cin):
    gen = torch.Generator().manual_seed((rows * 4099 + cout) * 4099 + cin + 1)
    return dict(g=torch.randint(-8, 9, (rows, cout), generator=gen).float(), w=torch.randint(-8, 9, (cout, cin), generator=gen).float())
