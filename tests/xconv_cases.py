"""Case table, restated dispatch rule and launch geometry, fp64 references and bounds of the kernel-level parity suite of csrc/xconv.hip
(tests/test_xconv_abi.py runs the cases on the GPU through the C ABI, tests/test_xconv_instantiations_cpu.py checks on any machine that
the cases reach every compiled kernel of xconv.hip, tests/test_xconv_cases_cpu.py checks this module itself).  A plain helper module:
nothing here imports the library.

Dispatch rule and launch geometry, restated from xconv.hip (NOT imported; kNumCU = 256, 256 threads = 4 waves per block):
  HF_DW_DISPATCH      (k, m) of hf_depthwise_k[_grad[_ws]]: (8,1) (8,2) (8,3) (8,4) (8,8) (4,1) (4,4)
  HF_XDW_DISPATCH     (k, m) of the fused entry points: (8,1) (8,2) (8,3) (8,4) (4,1) (4,4) (12,1) (12,2); hf_xconv_apply[_grad]: k in {4, 8}
  narrow / wide       c <= 64 and k m <= 64: depthwise_narrow_kernel<K, M, DX> (forward, input gradient) on narrow_grid: a multiple of
                      c / gcd(c, 256) blocks, at most 2048 before rounding up; else depthwise_fwd_kernel / depthwise_dx_kernel on
                      grid_for(rows c, 256): a thread takes a second (row, channel) pair past 2048 x 256 = 524 288 pairs
  dw_chunks           depthwise_dw_kernel: grid (ceil(c / 256) or 1, row chunks); chunks = min(ceil(512 / cblocks), ceil(rows / 64), rows,
                      65535), at least 1.  In a block cw = min(c, 256) channels x nrs = 256 / cw row slots; the slots of a channel meet by
                      "one_slot" (nrs == 1: nothing to meet), "shuffle" (cw a power of two <= 32: xor-shuffles, then the four waves in
                      LDS in a fixed order) or "lds" (the row slots take turns on one LDS slot per coefficient)
  grid_for            min(max(ceil(items / per_block), 1), 2048): xconv_apply_kernel, xconv_dx_kernel, xconv_dw_bwd_x_kernel walk rows with
                      4 waves per block: a wave takes a second row past 8192 rows
  xdw_grid            (rows, c, blocks per CU, channels per block column): column chunks cch = ceil(c / chunk), row chunks
                      min(ceil(blocks_per_cu 256 / cch), ceil(rows / 4)), rows per block = ceil(rows / row chunks)
  xdw_pair_grid       forward: xdw_grid(rows, c, 8, 128); a block has more than 4 rows only past 4 ceil(2048 / ceil(c / 128)) rows, and
                      its waves take a second trip (kXcRows = 2 rows in flight, 8 rows per trip) only past 8 rows per block
  xdw_bwd_grid        xconv_dw_bwd_fw_kernel: xdw_grid(rows, c, 4, 64), and rows per block raised to 32 when rows > 32
  xdw_v2              forward V2 (8-byte pair accesses): c even and f, fts, out 8-byte aligned
  xdw_table_grad      xconv_dw_bwd_fts_kernel<K, M, VEC>: xdw_grid(b n_src, c1, 8, 64 CPL), CPL = 4 for m = 1 else 2;
                      VEC = c1 % CPL == 0 and grad_out, grad_fts 16-byte aligned.  A wave walks kFtsRows = 2 table rows, kFtsEntries = 4
                      list entries of each per trip; a second trip over table rows needs more than 8 rows per block
  xdw_fts_direct      with a workspace: direct (rebuilt per table row) iff rows_per_cloud k >= 8 n_src, or the staged block
                      rows k c1 4 bytes <= 8 MiB, or m <= 2 and the block >= 80 MiB; else staged (xconv_dw_bwd_fw_kernel writes the
                      gathered block's gradient to the workspace, hf_group_point_grad_gather sums it).  Without a workspace: direct
  workspace           [round_up(4 b rows_per_cloud k c1, 256) bytes: staged block][4 grid.x k (c0 + c1) m: partial weight gradients],
                      grid.x of xdw_bwd_grid; hf_depthwise_k_grad_workspace = 4 nchunks k c m

References (fp64 numpy, from the formulas of include/hfops.h, never from the kernels), F = [F_delta | fts[cloud(r)][idx[r][j]]]:
  out[r][ch m' + m]   = sum_k (sum_j X[r][k][j] F[r][j][ch]) Wd[k][ch][m]
  dFX[r][k][ch]       = sum_m grad_out[r][ch M + m] Wd[k][ch][m]
  grad_x[r][k][j]     = sum_ch dFX[r][k][ch] F[r][j][ch]
  dF[r][j][ch]        = sum_k X[r][k][j] dFX[r][k][ch]           grad_f / grad_f_delta: the channels below c0
  grad_wd[k][ch][m]   = sum_r (sum_j X[r][k][j] F[r][j][ch]) grad_out[r][ch M + m]
  grad_fts[s][ch]     = sum over the (r, j) with idx[r][j] = s of dF[r][j][c0 + ch]          (a scatter-add over idx)
  hf_xconv_apply: out = X F; its gradients dF = X^T dO, dX = dO F^T.  hf_depthwise_k: y[r][ch M + m] = sum_w x[r][w][ch] W[w][ch][m];
  dx[r][w][ch] = sum_m dy[r][ch M + m] W[w][ch][m]; dW[w][ch][m] = sum_r x[r][w][ch] dy[r][ch M + m].

Two families of inputs.
EXACT: integers in [-A, A] (A = 2) in X, F_delta, the table, Wd and grad_out.  Every partial sum of every output is an integer of
magnitude at most exact_worst(case) = A^3 max(K K, c M, K M, rows K, longest list K M) (A^2 max(K, c, M, rows) for the two-kernel
entry points), asserted below 2^24: the fp32 result equals fp64 bit for bit whatever the order of the adds, the atomics, the DPP quad
sums and both table-gradient routes included.  This family sees a dropped row, a wrong block edge, a misrouted channel; it alone reaches
every kernel.
ROUND: seeded normals; every element within n u M of fp64 (gamma_n = n u / (1 - n u) to be exact), u = 2^-24, M the fp64 sum of the
magnitudes of the element's terms (the reference formula on absolute values), n the number of fp32 roundings on the longest path,
from the code's add order (a sum started at 0 takes its first term exactly; atomics: any order of T terms is at most T - 1 roundings):
  out         the K products and K - 1 adds of F_X, its product with Wd, K - 1 adds:                                  n = 2 K
  dF          dFX: M products, M - 1 adds; K products with X, K - 1 adds:                                            n = M + K
  grad_x      dFX (M), its product with F (1), a lane's ceil(c / 64) channels (ceil(c / 64) - 1 adds), the quad (2 adds), the 16 quad
              sums (15):                                                                                            n = M + ceil(c / 64) + 17
  grad_wd     F_X (K), its product with grad_out (1), a wave's ceil(rpb / 4) rows (- 1), the 4 waves of the block (3), the blocks:
              with a workspace ceil(gx / 16) - 1 + 15 (wgrad_reduce_kernel: 16 groups stride the chunks, then meet in order), without
              gx - 1 (global atomics, any order):                                       n = K + ceil(rpb / 4) + 3 + blocks term
  grad_fts    per table row with a list of L entries: dF (M + K) and L - 1 adds, the same on both routes:         n = M + K + L - 1
  apply       out, dF: n = K;  dX: 1 product, ceil(c / 64) - 1 adds, 63 adds over the lanes:                        n = ceil(c / 64) + 63
  depthwise   y: n = K;  dx: n = M;  dW: 1 product, a row slot's ceil(rpc / nrs) rows (- 1), the nrs slots of the block (at most
              nrs - 1, whichever way they meet), the chunks as grad_wd's blocks:        n = ceil(rpc / nrs) + nrs - 1 + chunks term
Nothing here is measured and nothing is tuned to the device."""
import zlib
from math import gcd

import numpy as np

from gemm_cases import U, cdiv  # noqa: F401

NUM_CU = 256
THREADS = 256
WAVES = THREADS // 64
XC_ROWS = 2
FTS_ROWS, FTS_ENTRIES = 2, 4
NARROW_MAX_C = 64
MAX_BLOCKS = 8 * NUM_CU
WRED_GROUPS = 16
DW_DISPATCH = ((8, 1), (8, 2), (8, 3), (8, 4), (8, 8), (4, 1), (4, 4))
XDW_DISPATCH = ((8, 1), (8, 2), (8, 3), (8, 4), (4, 1), (4, 4), (12, 1), (12, 2))
APPLY_K = (4, 8)
EXACT_A = 2
EXACT_LIMIT = 1 << 24
MIB = 1 << 20


def gam(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------- restated launch geometry
def grid_for(items, per_block):
    return min(max(cdiv(items, per_block), 1), MAX_BLOCKS)


def is_narrow(c, k, m):
    return c <= NARROW_MAX_C and k * m <= 64


def narrow_grid(rows, c):
    unit = c // gcd(c, THREADS)
    g = min(cdiv(rows * c, THREADS), MAX_BLOCKS)
    return cdiv(g, unit) * unit


def dw_chunks(rows, c):
    """(channel blocks, rows per chunk, chunks) of depthwise_dw_kernel"""
    cblocks = 1 if c < THREADS else cdiv(c, THREADS)
    chunks = cdiv(2 * NUM_CU, cblocks)
    chunks = max(min(chunks, cdiv(rows, 64)), 1)
    chunks = min(chunks, rows, 65535)
    rpc = cdiv(rows, chunks)
    return cblocks, rpc, cdiv(rows, rpc)


def dw_slots(c):
    cw = min(c, THREADS)
    return cw, THREADS // cw


def dw_reduction(c):
    cw, nrs = dw_slots(c)
    if nrs == 1:
        return "one_slot"
    return "shuffle" if cw & (cw - 1) == 0 and cw <= 32 else "lds"


def xdw_grid(rows, c, per_cu=8, chunk=64):
    """(grid.x, grid.y, rows per block)"""
    cch = cdiv(c, chunk)
    rch = cdiv(per_cu * NUM_CU, cch)
    rch = max(min(rch, cdiv(rows, 4)), 1)
    rpb = cdiv(rows, rch)
    return cdiv(rows, rpb), cch, rpb


def xdw_pair_grid(rows, c):
    return xdw_grid(rows, c, 8, 128)


def xdw_bwd_grid(rows, c):
    gx, gy, rpb = xdw_grid(rows, c, 4)
    if rpb < 32 and rows > 32:
        rpb = 32
        gx = cdiv(rows, rpb)
    return gx, gy, rpb


def fts_cpl(m):
    return 4 if m == 1 else 2


def fts_grid(src_rows, c1, m):
    return xdw_grid(src_rows, c1, 8, 64 * fts_cpl(m))


def xdw_v2(c, aligned):
    return c % 2 == 0 and aligned


def fts_vec(c1, m, aligned):
    return c1 % fts_cpl(m) == 0 and aligned


def staged_bytes(rows, k, c1):
    return 4 * rows * k * c1


def xdw_fts_direct(rows, n_src, p, k, c1, m):
    if p * k >= 8 * n_src:
        return True
    s = staged_bytes(rows, k, c1)
    return s <= 8 * MIB or (m <= 2 and s >= 80 * MIB)


def offsets_fit(rows, k, c, src_rows, c1=None):
    """xdw_offsets_fit: the forward kernel's 32-bit element offsets (the table is tested with the full width c, as the code does)"""
    return rows * k * c < 1 << 32 and src_rows * c < 1 << 32


def gathered_bytes(b, p, k, c1):
    return (4 * b * p * k * c1 + 255) & ~255


def gather_grad_workspace(b, p, k, c0, c1, m):
    if min(b, p, k, c0, c1, m) <= 0:
        return 0
    gx, _, _ = xdw_bwd_grid(b * p, c0 + c1)
    return gathered_bytes(b, p, k, c1) + 4 * gx * k * (c0 + c1) * m


def dw_grad_workspace(rows, k, c, m):
    if min(rows, k, c, m) <= 0:
        return 0
    return 4 * dw_chunks(rows, c)[2] * k * c * m


# ---------------------------------------------------------------------------------------------- cases
def _case(kind, family, regime, **kw):
    c = dict(kind=kind, family=family, regime=regime, off=())
    c.update(kw)
    return c


def case_id(c):
    parts = [c["kind"], c["family"], c["regime"], "k%dm%d" % (c["k"], c.get("m", 0))]
    if c["kind"] in ("fwd", "bwd"):
        parts += ["gather" if c["gather"] else "dense", "b%dp%dn%d" % (c["b"], c["p"], c["n"]), "c%d+%d" % (c["c0"], c["c1"])]
    else:
        parts += ["rows%d" % c["rows"], "c%d" % c["c"]]
    if c.get("want"):
        parts.append("want_" + "_".join(c["want"]))
    if "ws" in c:
        parts.append("ws" if c["ws"] else "nows")
    if c["off"]:
        parts.append("off_" + "_".join(c["off"]))
    return "-".join(parts)


def rows_of(c):
    return c["b"] * c["p"] if c["kind"] in ("fwd", "bwd") else c["rows"]


ALL4 = ("x", "f", "wd", "fts")


def _fused(kind, family, regime, k, m, gather, b, p, n, c0, c1, **kw):
    c = _case(kind, family, regime, k=k, m=m, gather=gather, b=b, p=p, n=n, c0=c0, c1=c1, **kw)
    if kind == "bwd":
        c.setdefault("want", ALL4 if gather else ALL4[:3])
        c.setdefault("ws", gather)
    return c


def _fwd_cases():
    out = []
    for fam in ("exact", "round"):
        for k, m in XDW_DISPATCH:
            for g in (True, False):
                out.append(_fused("fwd", fam, "block4", k, m, g, 3, 7, 13, 64, 70))        # 21 rows: blocks of 4, the last one of 1
                out.append(_fused("fwd", fam, "c_odd", k, m, g, 5, 3, 4, 64, 7))           # V2 off by parity; rows_per_cloud 3
    for k, m in XDW_DISPATCH:
        for g in (True, False):
            out.append(_fused("fwd", "exact", "trips", k, m, g, 243, 7, 5, 64, 1216))      # 1701 rows x 1280 channels: 9 rows per block
    out.append(_fused("fwd", "round", "trips", 8, 1, True, 243, 7, 5, 64, 1216))
    for k, m in ((8, 1), (8, 2), (4, 4), (12, 1)):
        out.append(_fused("fwd", "exact", "cloud1", k, m, True, 9, 1, 3, 64, 6))           # every row its own cloud
        out.append(_fused("fwd", "exact", "cloud3_trips", k, m, True, 620, 3, 2, 64, 1216))
    for k, m in ((8, 1), (12, 2)):
        for g, names in ((True, ("f", "fts", "out")), (False, ("f", "out"))):
            for name in names:
                out.append(_fused("fwd", "exact", "v2_off_align", k, m, g, 3, 7, 13, 64, 70, off=(name,)))
    for k, m in ((8, 3), (4, 1)):
        out.append(_fused("fwd", "exact", "straddle64", k, m, True, 3, 7, 13, 64, 200))    # the wave of block column 0 straddles channel 64
        out.append(_fused("fwd", "exact", "straddle192", k, m, True, 3, 7, 13, 192, 64))   # block column 1 (128..255) straddles 192
    for k, m in ((8, 4), (12, 1)):
        out.append(_fused("fwd", "exact", "c1_one", k, m, True, 3, 7, 13, 64, 1))
    return out


SUBSETS = (("x",), ("f",), ("wd",), ("fts",), ALL4)


def _bwd_cases():
    out = []
    for fam in ("exact", "round"):
        for k, m in XDW_DISPATCH:
            out.append(_fused("bwd", fam, "rows_le_32", k, m, True, 3, 7, 13, 64, 36))       # 21 rows in blocks of 4 (no floor), c = 100: dead lanes; VEC on
            out.append(_fused("bwd", fam, "rows_le_32", k, m, False, 3, 7, 13, 64, 36))
            out.append(_fused("bwd", fam, "vec_off_c1", k, m, True, 3, 7, 13, 64, 37))      # c1 % CPL != 0
    out.append(_fused("bwd", "exact", "rows_32", 8, 1, True, 4, 8, 5, 64, 36))                 # the last row count without the floor
    out.append(_fused("bwd", "exact", "single_block", 8, 2, True, 1, 3, 2, 64, 36))
    for k, m in XDW_DISPATCH:
        out.append(_fused("bwd", "exact", "floor32", k, m, True, 11, 3, 4, 64, 36))         # 33 rows: 32 + 1
    for k, m in ((8, 1), (8, 2), (4, 4), (12, 2)):
        out.append(_fused("bwd", "exact", "go_off", k, m, True, 3, 7, 13, 64, 36, off=("go",)))      # load_m's scalar branch, VEC off
        out.append(_fused("bwd", "exact", "go_off", k, m, False, 3, 7, 13, 64, 36, off=("go",)))
    out.append(_fused("bwd", "exact", "gfts_off", 8, 1, True, 3, 7, 13, 64, 36, off=("gfts",)))
    for k, m, g in ((8, 1, True), (8, 2, True), (4, 1, False)):
        out.append(_fused("bwd", "exact", "ragged_blocks", k, m, g, 243, 7, 5, 64, 1216))   # 1701 rows: 33 per block, the last one 18
    out.append(_fused("bwd", "round", "ragged_blocks", 8, 1, True, 243, 7, 5, 64, 1216))
    for k, m, g, c0, c1 in ((8, 1, True, 64, 4), (4, 4, True, 64, 4), (12, 1, True, 64, 4), (8, 2, False, 0, 8)):
        out.append(_fused("bwd", "exact", "rows_gt_8192", k, m, g, 1025, 8, 9, c0, c1))     # 8200 rows
    for k, m in ((8, 2), (4, 1)):
        for want in SUBSETS:
            for ws in (True, False):
                out.append(_fused("bwd", "exact", "subset", k, m, True, 3, 7, 13, 64, 36, want=want, ws=ws))
        for want in SUBSETS[:3]:
            out.append(_fused("bwd", "exact", "subset", k, m, False, 3, 7, 13, 64, 36, want=want))
    for ws in (True, False):
        out.append(_fused("bwd", "exact", "no_rows", 8, 1, True, 2, 0, 3, 64, 36, want=("wd", "fts"), ws=ws))
    # the table gradient
    for k, m, c1 in ((8, 1, 2048), (8, 2, 2048), (12, 2, 2048), (4, 4, 2048)):
        b = 4 * cdiv(MAX_BLOCKS, cdiv(c1, 64 * fts_cpl(m))) + 38                            # n_src = 2: just past 8 table rows per block
        out.append(_fused("bwd", "exact", "table_trips", k, m, True, b, 2, 2, 64, c1, want=("fts",), ws=False))
    out.append(_fused("bwd", "round", "table_trips", 8, 2, True, 550, 2, 2, 64, 2048, want=("fts",), ws=False))
    for n in (1, 2, 3):
        out.append(_fused("bwd", "exact", "n_src_small", 8, 1, True, 5, 3, n, 64, 36, want=("fts",), ws=False))
        out.append(_fused("bwd", "exact", "n_src_small", 12, 2, True, 5, 3, n, 64, 36, want=("fts",), ws=True))
    # routes with a workspace: both sides of each threshold of xdw_fts_direct
    for k, m, b, p, n, c1, regime in ((8, 1, 4, 1024, 1100, 68, "staged"), (4, 4, 4, 1024, 600, 132, "staged"), (12, 2, 8, 342, 600, 64, "staged"),
                                      (8, 1, 4, 1024, 1100, 64, "direct_8MiB"), (8, 1, 4, 1024, 1024, 68, "direct_lists_of_8"),
                                      (8, 1, 4, 1024, 1025, 68, "staged_lists_below_8"),
                                      (8, 2, 20, 1024, 1100, 128, "direct_80MiB"), (8, 2, 20, 1024, 1100, 124, "staged_below_80MiB")):
        out.append(_fused("bwd", "exact", regime, k, m, True, b, p, n, 64, c1, want=("fts", "wd"), ws=True))
    out.append(_fused("bwd", "round", "staged", 8, 1, True, 4, 1024, 1100, 64, 68, want=("fts", "wd"), ws=True))
    return out


def _two(kind, family, regime, k, m, rows, c, **kw):
    return _case(kind, family, regime, k=k, m=m, rows=rows, c=c, **kw)


DW_SWEEP_C = ((1, 2, 8, 32), (3, 24, 64, 100, 128), (129, 256, 257, 640))
DW_SWEEP_ROWS = (1, 63, 65, 203)


def _two_kernel_cases():
    out = []
    for k in APPLY_K:
        for c in (1, 63, 64, 65, 320):
            out.append(_two("apply", "exact", "rows_gt_8192", k, 0, 8200, c))
            out.append(_two("apply_grad", "exact", "rows_gt_8192", k, 0, 8200, c, want=("x", "f")))
        for fam in ("exact", "round"):
            out.append(_two("apply", fam, "small", k, 0, 37, 100))
            out.append(_two("apply_grad", fam, "small", k, 0, 37, 100, want=("x", "f")))
        out.append(_two("apply_grad", "exact", "small", k, 0, 37, 100, want=("x",)))
        out.append(_two("apply_grad", "exact", "small", k, 0, 37, 100, want=("f",)))
    for i, (k, m) in enumerate(DW_DISPATCH):
        for c in (3, 7, 24, 60):
            out.append(_two("dw", "exact", "narrow", k, m, 65, c))
            out.append(_two("dw_grad", "exact", "narrow", k, m, 65, c, want=("x", "w"), ws=bool(c & 4)))
        cn = (3, 7, 24, 60)[i % 4]
        rows = MAX_BLOCKS * THREADS // cn + 700                                              # the grid cap: a thread walks a second row
        out.append(_two("dw", "exact", "narrow_loop", k, m, rows, cn))
        out.append(_two("dw_grad", "exact", "narrow_loop", k, m, rows, cn, want=("x", "w"), ws=True))
        for fam in ("exact", "round"):
            out.append(_two("dw", fam, "wide", k, m, 63, 65))
            out.append(_two("dw_grad", fam, "wide", k, m, 63, 65, want=("x", "w"), ws=fam == "exact"))
            out.append(_two("dw", fam, "narrow_small", k, m, 130, 8))
            out.append(_two("dw_grad", fam, "narrow_small", k, m, 130, 8, want=("x", "w"), ws=fam == "exact"))
        out.append(_two("dw", "exact", "wide_loop", k, m, 4100, 129))                        # 528 900 pairs > 524 288
        out.append(_two("dw_grad", "exact", "wide_loop", k, m, 4100, 129, want=("x", "w"), ws=False))
    out.append(_two("dw_grad", "exact", "want_x", 8, 8, 65, 8, want=("x",), ws=False))
    out.append(_two("dw_grad", "exact", "want_x", 8, 2, 65, 100, want=("x",), ws=True))
    n = 0
    for group in DW_SWEEP_C:
        for c in group:
            for rows in DW_SWEEP_ROWS:
                for ws in (True, False):
                    k, m = DW_DISPATCH[n % len(DW_DISPATCH)]
                    n += 1
                    out.append(_two("dw_grad", "exact", "dw_" + dw_reduction(c), k, m, rows, c, want=("w",), ws=ws))
                    if rows == 203 and c in (8, 100, 257):
                        out.append(_two("dw_grad", "round", "dw_" + dw_reduction(c), k, m, rows, c, want=("w",), ws=ws))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _fwd_cases() + _bwd_cases() + _two_kernel_cases()
    return _CASES


def cases_of(*kinds):
    return [c for c in all_cases() if c["kind"] in kinds]


def aligned(c, *names):
    return not any(n in c["off"] for n in names)


def route(c):
    """'direct' / 'staged' / None of a gather-form backward case"""
    if c["kind"] != "bwd" or not c["gather"] or "fts" not in c["want"] or rows_of(c) == 0:
        return None
    if not c["ws"]:
        return "direct"
    return "direct" if xdw_fts_direct(rows_of(c), c["n"], c["p"], c["k"], c["c1"], c["m"]) else "staged"


def instantiations(c):
    """the (kernel, template arguments) the case launches"""
    k, m, kind = c["k"], c.get("m", 0), c["kind"]
    rows = rows_of(c)
    if rows == 0:
        return set()
    s = set()
    if kind == "fwd":
        names = ("f", "fts", "out") if c["gather"] else ("f", "out")
        s.add(("xconv_dw_fwd_kernel", (k, m, c["gather"], xdw_v2(c["c0"] + c["c1"], aligned(c, *names)), False)))    # BN off: xconv.hip
    elif kind == "bwd":
        want, g = c["want"], c["gather"]
        if {"f", "wd"} & set(want) or route(c) == "staged":
            s.add(("xconv_dw_bwd_fw_kernel", (k, m, g, False)))
        if "x" in want:
            s.add(("xconv_dw_bwd_x_kernel", (k, m, g)))
        if route(c) == "direct":
            s.add(("xconv_dw_bwd_fts_kernel", (k, m, fts_vec(c["c1"], m, aligned(c, "go", "gfts")))))
    elif kind == "apply":
        s.add(("xconv_apply_kernel", (k, False)))
    elif kind == "apply_grad":
        if "f" in c["want"]:
            s.add(("xconv_apply_kernel", (k, True)))
        if "x" in c["want"]:
            s.add(("xconv_dx_kernel", (k,)))
    elif kind == "dw":
        s.add(("depthwise_narrow_kernel", (k, m, False)) if is_narrow(c["c"], k, m) else ("depthwise_fwd_kernel", (k, m)))
    elif kind == "dw_grad":
        if "x" in c["want"]:
            s.add(("depthwise_narrow_kernel", (k, m, True)) if is_narrow(c["c"], k, m) else ("depthwise_dx_kernel", (k, m)))
        if "w" in c["want"]:
            s.add(("depthwise_dw_kernel", (k, m)))
    return s


def selected_instantiations(cases=None):
    s = set()
    for c in (all_cases() if cases is None else cases):
        s |= instantiations(c)
    return s


def exact_worst(c):
    """the largest magnitude any partial sum of any output of an exact case can reach"""
    a, k, m, rows = EXACT_A, c["k"], c.get("m", 1), rows_of(c)
    if c["kind"] in ("fwd", "bwd"):
        ch = c["c0"] + c["c1"]
        return a ** 3 * max(k * k, ch * m, k * m, rows * k, c["p"] * k * k * m)
    return a ** 2 * max(k, c["c"], m, rows)


# ---------------------------------------------------------------------------------------------- inputs
def _seed(c):
    return zlib.crc32(case_id(dict(c, family="any")).encode())


def _ladder(n, slots):
    """one cloud's slots: table row i is named (0, 1, 4, 5, 8, 9)[i % 6] times, what is left over goes to the last row but one"""
    flat = []
    for i in range(n):
        flat += [i] * (0, 1, 4, 5, 8, 9)[i % 6]
    flat = flat[:slots]
    return flat + [max(n - 2, 0)] * (slots - len(flat))


def make_idx(c, rng):
    """(b, p, k) neighbour table.  Forward: random, with table rows 0 and n - 1 named in the first and the last row of the first and the last
    cloud.  Backward with b >= 3 and n >= 12: cloud 0 names one table row in every slot, cloud 1 holds lists of 0, 1, 4, 5, 8 and 9 entries
    (around kFtsEntries = 4) in shuffled slots, the last cloud leaves its last table row unnamed; else random"""
    b, p, k, n = c["b"], c["p"], c["k"], c["n"]
    idx = rng.integers(0, n, (b, p, k)).astype(np.int32)
    if b == 0 or p == 0:
        return idx
    if c["kind"] == "fwd":
        for cloud in (0, b - 1):
            idx[cloud, 0, 0], idx[cloud, 0, k - 1], idx[cloud, p - 1, 0], idx[cloud, p - 1, k - 1] = 0, n - 1, n - 1, 0
    elif b >= 3 and n >= 12:
        idx[0] = min(7, n - 1)
        idx[1] = np.asarray(_ladder(n, p * k), np.int32)[rng.permutation(p * k)].reshape(p, k)
        idx[b - 1][idx[b - 1] == n - 1] = 0
    return idx


def index_inverse(idx, n):
    """the CSR inverse of include/hfops.h: offsets (b, n + 1), entries (b, p k): per table row the flat positions that name it, ascending"""
    b = idx.shape[0]
    flat = idx.reshape(b, -1)
    offsets = np.zeros((b, n + 1), np.int32)
    entries = np.zeros(flat.shape, np.int32)
    for i in range(b):
        offsets[i, 1:] = np.cumsum(np.bincount(flat[i], minlength=n))
        entries[i] = np.argsort(flat[i], kind="stable")
    return offsets, entries


def list_lengths(idx, n):
    b = idx.shape[0]
    return np.stack([np.bincount(idx[i].reshape(-1), minlength=n) for i in range(b)]) if b else np.zeros((0, n), np.int64)


def make_inputs(c):
    """float32 / int32 numpy arrays of the case"""
    rng = np.random.default_rng(_seed(c))
    exact = c["family"] == "exact"
    draw = (lambda *s: rng.integers(-EXACT_A, EXACT_A + 1, s).astype(np.float32)) if exact else (lambda *s: rng.standard_normal(s, np.float32))
    k, m, rows = c["k"], c.get("m", 0), rows_of(c)
    if c["kind"] in ("fwd", "bwd"):
        b, n, c0, c1 = c["b"], c["n"], c["c0"], c["c1"]
        t = dict(x=draw(rows, k, k), fd=draw(rows, k, c0), fts=draw(b * n, c1), wd=draw(k, c0 + c1, m), idx=make_idx(c, rng))
        if c["kind"] == "bwd":
            t["go"] = draw(rows, (c0 + c1) * m)
            t["offsets"], t["entries"] = index_inverse(t["idx"], n)
        return t
    ch = c["c"]
    if c["kind"] in ("apply", "apply_grad"):
        t = dict(x=draw(rows, k, k), f=draw(rows, k, ch))
        if c["kind"] == "apply_grad":
            t["go"] = draw(rows, k, ch)
        return t
    t = dict(x=draw(rows, k, ch), w=draw(k, ch, m))
    if c["kind"] == "dw_grad":
        t["go"] = draw(rows, ch * m)
    return t


# ---------------------------------------------------------------------------------------------- references
def _d(a):
    return np.asarray(a, np.float64)


def concat_f(c, t, mag=False):
    """F = [F_delta | gathered table rows] (rows, k, c0 + c1) in fp64"""
    b, p, n = c["b"], c["p"], c["n"]
    rows = b * p
    table_row = (np.arange(b)[:, None, None] * n + t["idx"]).reshape(rows, c["k"])
    f = np.concatenate([_d(t["fd"]), _d(t["fts"])[table_row]], axis=2)
    return np.abs(f) if mag else f


def scatter_add(values, target, n):
    """(n, width): row s is the sum of the rows of `values` whose target is s"""
    order = np.argsort(target, kind="stable")
    counts = np.bincount(target, minlength=n)
    out = np.zeros((n, values.shape[1]))
    named = counts > 0
    if named.any():
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        out[named] = np.add.reduceat(values[order], starts[named], axis=0)
    return out


def ref_fused_fwd(c, t, mag=False):
    a = np.abs if mag else (lambda v: v)
    fx = np.matmul(a(_d(t["x"])), concat_f(c, t, mag))                        # (rows, k, c)
    return np.einsum("rkc,kcm->rcm", fx, a(_d(t["wd"]))).reshape(fx.shape[0], -1)


def ref_fused_bwd(c, t, want, mag=False):
    """dict of the wanted gradients: x (rows, k, k), f (rows, k, c0 for the gather form, c for the dense one), wd (k, c, m), fts (b n, c1)"""
    a = np.abs if mag else (lambda v: v)
    k, m, c0, c1, b, n = c["k"], c["m"], c["c0"], c["c1"], c["b"], c["n"]
    rows = b * c["p"]
    x, wd, f = a(_d(t["x"])), a(_d(t["wd"])), concat_f(c, t, mag)
    g = a(_d(t["go"])).reshape(rows, c0 + c1, m)
    out = {}
    if "wd" in want:
        out["wd"] = np.einsum("rkc,rcm->kcm", np.matmul(x, f), g)
    if {"x", "f", "fts"} & set(want):
        dfx = np.einsum("rcm,kcm->rkc", g, wd)
        if "x" in want:
            out["x"] = np.matmul(dfx, f.transpose(0, 2, 1))
        if {"f", "fts"} & set(want):
            if c["gather"] and "f" not in want:
                dfx = dfx[:, :, c0:]
                df = np.matmul(x.transpose(0, 2, 1), dfx)
                lo = 0
            else:
                df = np.matmul(x.transpose(0, 2, 1), dfx)
                lo = c0
            if "f" in want:
                out["f"] = df[:, :, :c0] if c["gather"] else df
            if "fts" in want:
                table_row = (np.arange(b)[:, None, None] * n + t["idx"]).reshape(-1)
                out["fts"] = scatter_add(df[:, :, lo:].reshape(rows * k, c1), table_row, b * n)
    return out


def ref_apply(t, mag=False):
    a = np.abs if mag else (lambda v: v)
    return np.matmul(a(_d(t["x"])), a(_d(t["f"])))


def ref_apply_grad(t, mag=False):
    a = np.abs if mag else (lambda v: v)
    x, f, g = a(_d(t["x"])), a(_d(t["f"])), a(_d(t["go"]))
    return dict(x=np.matmul(g, f.transpose(0, 2, 1)), f=np.matmul(x.transpose(0, 2, 1), g))


def ref_dw(t, mag=False):
    a = np.abs if mag else (lambda v: v)
    y = np.einsum("rwc,wcm->rcm", a(_d(t["x"])), a(_d(t["w"])))
    return y.reshape(y.shape[0], -1)


def ref_dw_grad(t, mag=False):
    a = np.abs if mag else (lambda v: v)
    x, w = a(_d(t["x"])), a(_d(t["w"]))
    g = a(_d(t["go"])).reshape(x.shape[0], w.shape[1], w.shape[2])
    return dict(x=np.einsum("rcm,wcm->rwc", g, w), w=np.einsum("rwc,rcm->wcm", x, g))


def _blocks_term(blocks, ws):
    return cdiv(blocks, WRED_GROUPS) - 1 + WRED_GROUPS - 1 if ws else blocks - 1


def roundings(c, t=None):
    """n of every output of the case (see the module docstring); fts: per table row, (b n, 1)"""
    k, m = c["k"], c.get("m", 0)
    rows = rows_of(c)
    if c["kind"] == "fwd":
        return dict(out=2 * k)
    if c["kind"] == "bwd":
        ch = c["c0"] + c["c1"]
        gx, _, rpb = xdw_bwd_grid(rows, ch)
        n = dict(x=m + cdiv(ch, 64) + 17, f=m + k, wd=k + cdiv(rpb, WAVES) + 3 + _blocks_term(gx, c["ws"]))
        if t is not None:
            n["fts"] = (m + k + np.maximum(list_lengths(t["idx"], c["n"]), 1) - 1).reshape(-1, 1).astype(np.float64)
        return n
    if c["kind"] == "apply":
        return dict(out=k)
    if c["kind"] == "apply_grad":
        return dict(f=k, x=cdiv(c["c"], 64) + 63)
    if c["kind"] == "dw":
        return dict(y=k)
    _, rpc, nchunks = dw_chunks(rows, c["c"])
    _, nrs = dw_slots(c["c"])
    return dict(x=m, w=cdiv(rpc, nrs) + nrs - 1 + _blocks_term(nchunks, c["ws"]))


def bound(n, mag):
    return gam(n) * mag
