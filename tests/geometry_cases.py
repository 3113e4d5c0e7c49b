"""Case table, restated dispatch rules and independent NumPy statements of the point-geometry kernels: farthest point sampling
(csrc/sampling.hip), ball query (csrc/grouping.hip, csrc/ballquery.hip, csrc/ballquery_sorted.hip), kNN and select_top_k
(csrc/grouping.hip).  tests/test_geometry_abi.py runs the cases on the GPU against the CPU oracle, tests/test_geometry_instantiations_cpu.py
checks on any machine that the cases reach every compiled kernel of the four sources, tests/test_geometry_cases_cpu.py checks this module
itself (the pinned constants, every case's regime, the oracle against the statements below, the sharpness of the inputs).  A plain helper
module: nothing here imports the library.

Dispatch rules, restated from the sources (NOT imported; the constants are pinned against the sources by test_geometry_cases_cpu.py):
  FPS      hf_farthest_point_sample[_variant] -> launch_fps_onchip (sampling.hip).  n > kFpsMaxPoints: fps_scratch_kernel whatever is
           forced.  wave (forced, or auto with n <= kFpsWaveMaxPoints): fps_wave_kernel<PPT>, PPT = ceil(n / 64) rounded up to 1 / 2 / 4 / 8,
           four clouds per 256-thread workgroup.  bucket (forced, or auto with n >= 8192 and m >= 256): fps_bucket_kernel<PPT, NT>, NT = 512
           unless threads == 1024, PPT = ceil(n / NT) rounded up to a power of two (at most 32 with 512 threads, 16 with 1024).  plain:
           fps_onchip_kernel<PPT, NT>, NT = threads, or 256 up to 4096 points and 512 beyond; the same PPT rule; 256 threads take at most
           4096 points (PPT <= 16), so fps_onchip_kernel<32, 256> is compiled and never launched.
  ball     launch_ball_query (grouping.hip): sorted forced, or auto with a workspace, b >= 32 and b ceil(m / 128) > kNumCU -> the cell-sorted
           pair; else the single-launch cell kernel; else (nsample > 128, n > 2^kCellIdxBits, radius out of range) the brute-force kernel.
           cell (ballquery.hip): qpw = 128 / 64 / 32 for nsample <= 32 / <= 64 / else; 256 when nsample <= 32 and b ceil(m / 256) >= kNumCU;
           halved while qpw > 16 and b ceil(m / qpw) < kNumCU.  Stores: write-through (2) when b ceil(m / qpw) <= kNumCU, else
           non-temporal (1).  A4: n % 4 == 0 and the cloud pointer 16-byte aligned.  qbp_cell_kernel<GROUP, SM, 1024, A4>.
           sorted (ballquery_sorted.hip): split = 4 / 2 / 1 for 4 b <= kNumCU / 2 b <= kNumCU / else; bq_build_kernel<PPT, HB, S>:
           n <= 1024 <1,10,1>; n <= 4096 <4,12,2> (split >= 2) or <4,12,1>; n <= 16384 <16,14,4> / <16,14,2> / <16,14,1> by split;
           beyond <0,14,4>.  Rows are packed (index << 16 | position) up to kPackedMaxN points.  bq_query_kernel<GROUP, 1, 8>.
  kNN      hf_knn_point: n <= 4096, k in {4, 8, 12, 16} and ceil(m / 256) b >= 256 -> knn_small_kernel<k>; else knn_kernel<PARTS>,
           PARTS = 1 from 262144 queries, 4 from 65536, else 16.  k <= n, and the lists (8 k 256 bytes) plus a 12 KB tile within 150 KB.
           hf_knn_point_sorted (launch_knn_grid; hf_three_nn_sorted calls it with k = 3): n > kKnnBinMaxData falls back to hf_knn_point;
           else knn_bin_kernel + knn_grid_reg_kernel<k> for k in {3, 4, 8, 12, 16}, knn_grid_kernel for any other k.
  top-k    hf_select_top_k: select_top_k_kernel.

Independent statements (NumPy, the fourth part of a case): the distance expression is evaluated in fp32 exactly as the reference writes it
(differences, squares, left-to-right sum; NumPy never contracts to FMA) and everything that ranks is done on those values:
  FPS      round j takes the point whose running minimum distance to the samples so far is largest; among equal distances the smallest
           (k mod 512, k) -- the reference's 512-thread strided scan and left-biased tree -- which is the lowest index up to 512 points
  ball     hit iff max(sqrtf(s), 1e-20f) < radius; a row holds the first nsample hits in ascending index padded with the first hit;
           pts_cnt = min(hits, nsample); a row without a hit is zeros
  kNN      the k smallest (distance, index) pairs, ascending
  top-k    the reference's selection sort: k passes, each swaps the FIRST minimum of the tail into place
Nothing here is measured and nothing is tuned to the device."""
import zlib

import numpy as np

# ---------------------------------------------------------------------------------------------- constants of the sources
NUM_CU = 256                   # hf_common.h kNumCU
FPS_MAX_POINTS = 16384         # sampling.hip kFpsMaxPoints (hf_fps_onchip_limit)
FPS_WAVE_MAX_POINTS = 512      # sampling.hip kFpsWaveMaxPoints
FPS_WAVE_THREADS = 256         # sampling.hip kFpsWaveThreads
FPS_TIE_MOD = 512              # sampling.hip fps_tiekey: k & 511
QB_THREADS, QB_TILE = 256, 1024            # grouping.hip kQbThreads, kQbTile
KNN_THREADS, KNN_TILE = 256, 1024          # grouping.hip kKnnThreads, kKnnTile
KNN_BIN_THREADS, KNN_MAX_GRID = 1024, 64   # grouping.hip kKnnBinThreads, kKnnMaxGrid
KNN_BIN_MAX_DATA = 65536       # grouping.hip kKnnBinMaxData
CELL_THREADS = 1024            # ballquery.hip: nt of launch_ball_query_cell
CELL_IDX_BITS = 19             # ballquery.hip kCellIdxBits
CELL_SEG_POINTS = 16384        # ballquery.hip kCellSegPoints
SORT_THREADS, QUERY_THREADS = 1024, 256    # ballquery_sorted.hip kSortThreads, kQueryThreads
PACKED_MAX_N = 32768           # ballquery_sorted.hip kPackedMaxN
SORTED_LANES = 8               # ballquery_sorted.hip: g of launch_ball_query_sorted

# (file, constant, value): read back from the definitions in the sources by test_geometry_cases_cpu.py
SOURCE_CONSTANTS = (
    ("hf_common.h", "kNumCU", NUM_CU), ("sampling.hip", "kFpsMaxPoints", FPS_MAX_POINTS), ("sampling.hip", "kFpsWaveMaxPoints", FPS_WAVE_MAX_POINTS),
    ("sampling.hip", "kFpsWaveThreads", FPS_WAVE_THREADS), ("grouping.hip", "kQbThreads", QB_THREADS), ("grouping.hip", "kQbTile", QB_TILE),
    ("grouping.hip", "kKnnThreads", KNN_THREADS), ("grouping.hip", "kKnnTile", KNN_TILE), ("grouping.hip", "kKnnBinThreads", KNN_BIN_THREADS),
    ("grouping.hip", "kKnnMaxGrid", KNN_MAX_GRID), ("grouping.hip", "kKnnBinMaxData", KNN_BIN_MAX_DATA), ("ballquery.hip", "kCellIdxBits", CELL_IDX_BITS),
    ("ballquery.hip", "kCellSegPoints", CELL_SEG_POINTS), ("ballquery_sorted.hip", "kSortThreads", SORT_THREADS),
    ("ballquery_sorted.hip", "kQueryThreads", QUERY_THREADS), ("ballquery_sorted.hip", "kPackedMaxN", PACKED_MAX_N),
)
# (file, text that must stand in the file): the literals of the rules that are no named constant
SOURCE_RULES = (
    ("sampling.hip", "(static_cast<unsigned>(k & 511) << 22)"),
    ("sampling.hip", "mode == 2 || (mode == 0 && n >= 8192 && m >= 256)"),
    ("sampling.hip", "if (nt != 1024 && n <= 512 * 32) return launch_fps_bucket_nt<512>"),
    ("sampling.hip", "if (nt == 0) nt = n <= 4096 ? 256 : 512;"),
    ("sampling.hip", "if (nt == 256 && n <= 256 * 16) return launch_fps_plain_nt<256>"),
    ("sampling.hip", "if (nt <= 512 && n <= 512 * 32) return launch_fps_plain_nt<512>"),
    ("grouping.hip", "workspace && b >= 32 && static_cast<long long>(b) * div_up(m, 128) > kNumCU"),
    ("grouping.hip", "if (lds > 160 * 1024) return HF_EINVAL;"),
    ("grouping.hip", "n <= 4096 && (k == 4 || k == 8 || k == 12 || k == 16) && static_cast<long long>(div_up(m, kKnnThreads)) * b >= 256"),
    ("grouping.hip", "if (queries >= 256 * 1024) HF_KNN_LAUNCH(1);"),
    ("grouping.hip", "else if (queries >= 64 * 1024) HF_KNN_LAUNCH(4);"),
    ("grouping.hip", "if (lds > 150 * 1024 || b > 65535) return HF_EINVAL;"),
    ("ballquery.hip", "HF_DIAG_INT(\"HF_QBP_NT\", 1024) == 512 ? 512 : 1024"),
    ("ballquery.hip", "int qpw = nsample <= 32 ? 128 : (nsample <= 64 ? 64 : 32);"),
    ("ballquery.hip", "if (nsample <= 32 && nt == 1024 && static_cast<long long>(b) * div_up(m, 256) >= kNumCU) qpw = 256;"),
    ("ballquery.hip", "while (qpw > nt / 64 && static_cast<long long>(b) * div_up(m, qpw) < kNumCU) qpw >>= 1;"),
    ("ballquery.hip", "static_cast<long long>(b) * div_up(m, qpw) <= kNumCU ? 2 : 1"),
    ("ballquery.hip", "(n % 4 == 0) && (reinterpret_cast<uintptr_t>(xyz1) % 16 == 0)"),
    ("ballquery_sorted.hip", "b * 4 <= kNumCU ? 4 : (b * 2 <= kNumCU ? 2 : 1)"),
    ("ballquery_sorted.hip", "static int bq_hbits(int n) { return n <= 1024 ? 10 : (n <= 4096 ? 12 : 14); }"),
    ("ballquery_sorted.hip", "HF_DIAG_INT(\"HF_BQ_G\", 8)"),
)

FPS_KERNELS = ("auto", "plain", "bucket", "wave")
BQ_VARIANTS = ("auto", "cell", "bruteforce", "sorted")

# dispatch tables: the template arguments each rule can produce
FPS_WAVE_PPT = (1, 2, 4, 8)
FPS_PLAIN_PPT = {256: (1, 2, 4, 8, 16), 512: (1, 2, 4, 8, 16, 32), 1024: (1, 2, 4, 8, 16)}
FPS_BUCKET_PPT = {512: (1, 2, 4, 8, 16, 32), 1024: (1, 2, 4, 8, 16)}
CELL_STORE_MODES = (1, 2)
CELL_QPW = (256, 128, 64, 32, 16)
BQ_BUILD = ((1, 10, 1), (4, 12, 2), (4, 12, 1), (16, 14, 4), (16, 14, 2), (16, 14, 1), (0, 14, 4))
KNN_SMALL_K = (4, 8, 12, 16)
KNN_PARTS = (1, 4, 16)
KNN_REG_K = (3, 4, 8, 12, 16)

# Compiled, never launched by the product build: HF_DIAG_INT(name, dflt) is the constant dflt without -DHF_DIAG (hf_common.h), so the
# restated rule cannot select them; they are NOT reached by building with -DHF_DIAG.  (kernel, template arguments, file, text of the line
# that makes it unreachable): the line is looked up in the file by test_geometry_cases_cpu.py.
_B = (False, True)
DIAGNOSTIC_ONLY = tuple(
    [("qbp_cell_kernel", (g, 0, nt, a4), "ballquery.hip", "const int sm = HF_DIAG_INT(\"HF_QBP_STORE\", static_cast<long long>(b) * div_up(m, qpw) <= kNumCU ? 2 : 1);")
     for g in _B for nt, a4 in ((1024, True), (1024, False), (512, False))] +
    [("qbp_cell_kernel", (g, sm, 512, False), "ballquery.hip", "const int nt = HF_DIAG_INT(\"HF_QBP_NT\", 1024) == 512 ? 512 : 1024;")
     for g in _B for sm in CELL_STORE_MODES] +
    [("bq_query_kernel", (g, 1, lanes), "ballquery_sorted.hip", "const int g = HF_DIAG_INT(\"HF_BQ_G\", 8);") for g in _B for lanes in (4, 2)] +
    # no diagnostic knob: 256 threads are only taken up to 256 * 16 points, where PPT <= 16 (the launcher's 32-point form needs NT <= 512)
    [("fps_onchip_kernel", (32, 256), "sampling.hip", "if (nt == 256 && n <= 256 * 16) return launch_fps_plain_nt<256>(b, n, m, inp, out, st);")])

# Kernels of the four sources that belong to families pinned elsewhere (the row-gather machine of row_gather.h: tests/test_row_gather_*;
# group_concat: test_ops_gpu.py): named one by one, not ignored by pattern.  (file, kernel, template arguments)
OUT_OF_SCOPE = (
    ("sampling.hip", "gather_rows_kernel", (1, 1, 3)), ("sampling.hip", "gather_rows_kernel", (1, 4, 0)), ("sampling.hip", "gather_rows_pow2_kernel", (1, 4)),
    ("sampling.hip", "scatter_rows_kernel", (1, 3)),
    ("grouping.hip", "gather_rows_kernel", (1, 1, 0)), ("grouping.hip", "gather_rows_kernel", (1, 4, 0)), ("grouping.hip", "gather_rows_pow2_kernel", (1, 4)),
    ("grouping.hip", "grad_gather_rows_kernel", (1, 1)), ("grouping.hip", "grad_gather_rows_kernel", (1, 4)), ("grouping.hip", "scatter_rows_kernel", (1, 0)),
    ("grouping.hip", "group_concat_kernel", ()),
)
SOURCES = ("sampling.hip", "grouping.hip", "ballquery.hip", "ballquery_sorted.hip")


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- restated dispatch
def _pow2_ppt(ppt, top):
    for p in (1, 2, 4, 8, 16, 32):
        if ppt <= p and p <= top:
            return p
    return None


def fps_dispatch(n, m, kernel="auto", threads=0):
    """(kernel, template arguments) of hf_farthest_point_sample (kernel 'auto', threads 0) or hf_farthest_point_sample_variant; None: HF_EINVAL"""
    assert kernel in FPS_KERNELS and threads in (0, 256, 512, 1024)
    if n > FPS_MAX_POINTS:
        return ("fps_scratch_kernel", ())
    if kernel == "wave" and n > FPS_WAVE_MAX_POINTS:
        return None
    if kernel == "plain" and threads and n > threads * (16 if threads == 1024 else 32):
        return None
    if kernel == "plain" and threads == 256 and n > 256 * 16:
        return None
    if kernel == "wave" or (kernel == "auto" and n <= FPS_WAVE_MAX_POINTS):
        ppt = cdiv(n, 64)
        return ("fps_wave_kernel", (1 if ppt <= 1 else 2 if ppt <= 2 else 4 if ppt <= 4 else 8,))
    if kernel == "bucket" or (kernel == "auto" and n >= 8192 and m >= 256):
        nt = 512 if threads != 1024 and n <= 512 * 32 else 1024
        p = _pow2_ppt(cdiv(n, nt), 32 if nt <= 512 else 16)
        return None if p is None else ("fps_bucket_kernel", (p, nt))
    nt = threads or (256 if n <= 4096 else 512)
    nt = 256 if nt == 256 and n <= 256 * 16 else 512 if nt <= 512 and n <= 512 * 32 else 1024
    p = _pow2_ppt(cdiv(n, nt), 32 if nt <= 512 else 16)
    return None if p is None else ("fps_onchip_kernel", (p, nt))


def fps_wave_grid(b):
    """workgroups of fps_wave_kernel: four clouds each"""
    return cdiv(b, FPS_WAVE_THREADS // 64)


def _radius_in_range(r):
    return 1.0e-18 < r < 3.0e18


def cell_geometry(b, m, nsample):
    """(queries per workgroup, store mode) of launch_ball_query_cell"""
    qpw = 128 if nsample <= 32 else 64 if nsample <= 64 else 32
    if nsample <= 32 and b * cdiv(m, 256) >= NUM_CU:
        qpw = 256
    while qpw > CELL_THREADS // 64 and b * cdiv(m, qpw) < NUM_CU:
        qpw >>= 1
    return qpw, (2 if b * cdiv(m, qpw) <= NUM_CU else 1)


def cell_dispatch(b, n, m, radius, nsample, group, aligned=True):
    if nsample > 128 or not _radius_in_range(radius) or b > 65535 or n > 1 << CELL_IDX_BITS:
        return None
    qpw, sm = cell_geometry(b, m, nsample)
    if cdiv(m, qpw) > 65535:
        return None
    return [("qbp_cell_kernel", (bool(group), sm, CELL_THREADS, n % 4 == 0 and aligned))]


def sorted_split(b):
    return 4 if b * 4 <= NUM_CU else 2 if b * 2 <= NUM_CU else 1


def sorted_build(b, n):
    split = sorted_split(b)
    if n <= 1024:
        return (1, 10, 1)
    if n <= 4096:
        return (4, 12, 2) if split >= 2 else (4, 12, 1)
    if n <= 16384:
        return (16, 14, 4) if split >= 4 else (16, 14, 2) if split == 2 else (16, 14, 1)
    return (0, 14, 4)


def sorted_dispatch(b, n, m, radius, nsample, group):
    if nsample > 128 or not _radius_in_range(radius) or b > 65535 or n > 1 << 26 or cdiv(m, QUERY_THREADS // SORTED_LANES) > 65535:
        return None
    return [("bq_build_kernel", sorted_build(b, n)), ("bq_query_kernel", (bool(group), 1, SORTED_LANES))]


def sorted_workspace(b, n):
    hbits = 10 if n <= 1024 else 12 if n <= 4096 else 14
    return b * ((16 * n + 4 * ((1 << hbits) + 4) + 15) // 16 * 16)


def bq_dispatch(variant, b, n, m, radius, nsample, group, ws=False, aligned=True):
    """the kernels launch_ball_query launches; None: HF_EINVAL.  ws: the caller passes a workspace (sorted needs one)"""
    assert variant in BQ_VARIANTS
    if variant == "sorted":
        assert ws
        return sorted_dispatch(b, n, m, radius, nsample, group)
    if variant == "auto" and ws and b >= 32 and b * cdiv(m, 128) > NUM_CU:
        s = sorted_dispatch(b, n, m, radius, nsample, group)
        if s is not None:
            return s
    if variant != "bruteforce":
        c = cell_dispatch(b, n, m, radius, nsample, group, aligned)
        if c is not None or variant == "cell":
            return c
    if 4 * QB_TILE * 3 + 4 * QB_THREADS * ((nsample | 1) + 1) > 160 * 1024:
        return None
    return [("qbp_bruteforce_kernel", (bool(group),))]


def wrapper_passes_workspace(variant, b, m):
    """heterofusionrcnn_amd/grouping.py _ball_query: when the Python wrapper allocates the cell-sorted workspace"""
    return variant == "sorted" or (variant == "auto" and b >= 32 and b * cdiv(m, 128) > 256)


def knn_dispatch(b, n, m, k):
    """hf_knn_point"""
    if k > n or 4 * KNN_TILE * 3 + 8 * k * KNN_THREADS > 150 * 1024 or b > 65535:
        return None
    if n <= 4096 and k in KNN_SMALL_K and cdiv(m, KNN_THREADS) * b >= 256:
        return [("knn_small_kernel", (k,))]
    q = b * m
    return [("knn_kernel", (1 if q >= 256 * 1024 else 4 if q >= 64 * 1024 else 16,))]


def knn_sorted_dispatch(b, n, m, k):
    """hf_knn_point_sorted; hf_three_nn_sorted is the same with k = 3 (n: the known points)"""
    if k > n:
        return None
    if n > KNN_BIN_MAX_DATA:
        return knn_dispatch(b, n, m, k)
    if 8 * k * KNN_THREADS > 150 * 1024 or b > 65535:
        return None
    return [("knn_bin_kernel", ()), ("knn_grid_reg_kernel", (k,)) if k in KNN_REG_K else ("knn_grid_kernel", ())]


def knn_grid_for(n):
    g = 4
    while g < KNN_MAX_GRID and g * g * 4 < n:
        g <<= 1
    return g


# ---------------------------------------------------------------------------------------------- cases
def _case(family, regime, **kw):
    c = dict(family=family, regime=regime)
    c.update(kw)
    return c


def case_id(c):
    f = c["family"]
    if f == "fps":
        return "fps-%s-%s%d-b%dn%dm%d" % (c["regime"], c["kernel"], c["threads"], c["b"], c["n"], c["m"])
    if f == "bq":
        return "bq-%s-%s-%s-b%dn%dm%d-ns%d%s%s" % (c["regime"], c["variant"], "group" if c["group"] else "idx", c["b"], c["n"], c["m"], c["nsample"],
                                                  "-ws" if c["ws"] else "", "-off" if c["off"] else "")
    if f == "knn":
        return "knn-%s-%s-b%dn%dm%dk%d" % (c["regime"], c["entry"], c["b"], c["n"], c["m"], c["k"])
    return "topk-%s-b%dm%dn%dk%d" % (c["regime"], c["b"], c["m"], c["n"], c["k"])


WAVE_N = (64, 65, 128, 129, 200, 256, 257, 512)      # PPT 1: 64; 2: 65, 128; 4: 129, 200, 256; 8: 257, 512
WAVE_M = {64: 100, 65: 33, 128: 130, 129: 64, 200: 300, 256: 255, 257: 64, 512: 129}
_M_CYCLE = (32, 150, 300, 77)


def _ppt_edges(p, nt, small):
    """the lengths of a PPT bucket: its lower edge plus one (no multiple of 64) and its upper edge; PPT 1: a short ragged cloud instead"""
    return (small if p == 1 else (p // 2) * nt + 1, p * nt)


def _fps_cases():
    out = []
    for n in WAVE_N:
        for b in (1, 5):      # four clouds share a workgroup: 5 leaves a ragged second one
            out.append(_case("fps", "wave", kernel="wave", threads=0, b=b, n=n, m=WAVE_M[n], same=3 if (b, n) == (5, 200) else None))
    i = 0
    for nt in (256, 512, 1024):
        for p in FPS_PLAIN_PPT[nt]:
            for n in _ppt_edges(p, nt, 229):
                m = 300 if n <= 256 else _M_CYCLE[i % 4]
                i += 1
                first = (nt, n) == (256, 513)
                out.append(_case("fps", "plain", kernel="plain", threads=nt, b=3 if first else 2, n=n, m=m, same=1 if first else None))
    for nt in (512, 1024):
        for p in FPS_BUCKET_PPT[nt]:
            for n in _ppt_edges(p, nt, 200):
                m = 300 if n <= 256 else _M_CYCLE[i % 4]
                i += 1
                first = (nt, n) == (512, 1025)
                out.append(_case("fps", "bucket", kernel="bucket", threads=nt, b=3 if first else 2, n=n, m=m, same=2 if first else None))
    out.append(_case("fps", "scratch", kernel="auto", threads=0, b=2, n=FPS_MAX_POINTS + 1, m=40, same=None))
    return out


def _bq(regime, variant, group, b, n, m, nsample, radius=0.4, center=True, ws=False, off=False, **want):
    return _case("bq", regime, variant=variant, group=group, b=b, n=n, m=m, nsample=nsample, radius=radius, center=center, ws=ws, off=off, want=want)


def _bq_cases():
    out = []
    for g in _B:
        out.append(_bq("tiles", "bruteforce", g, 2, 1030, 300, 16))                      # two LDS tiles of data (1024 + 6), two blocks of queries
        out.append(_bq("ns_gt_128", "auto", g, 2, 600, 70, 140, center=not g))            # outside the cell kernel's range: auto lands here
    # the single-launch cell kernel: GROUP x store mode x A4
    for g in _B:
        for sm in CELL_STORE_MODES:
            for a4 in _B:
                b, m = (129, 130) if sm == 1 else (2, 70)
                n = (300 if sm == 1 else 1000) + (0 if a4 else 1)
                out.append(_bq("cube", "cell", g, b, n, m, 32, center=a4, sm=sm, a4=a4, qpw=128 if sm == 1 else 16))
    # a cloud pointer 4 bytes past a 16-byte boundary, through the C ABI, n a multiple of 4: A4 off by alignment alone
    out.append(_bq("ptr_off", "cell", True, 2, 1000, 70, 32, off=True, sm=2, a4=False, qpw=16))
    out.append(_bq("ptr_off", "cell", False, 129, 300, 130, 32, off=True, sm=1, a4=False, qpw=128))
    # queries per workgroup and nsample
    out.append(_bq("qpw", "cell", True, 256, 128, 200, 32, sm=2, a4=True, qpw=256))
    out.append(_bq("qpw", "cell", False, 130, 129, 257, 7, sm=1, a4=False, qpw=256))
    out.append(_bq("qpw", "cell", True, 128, 128, 130, 32, sm=2, a4=True, qpw=128))
    out.append(_bq("qpw", "cell", True, 64, 300, 200, 64, sm=2, a4=True, qpw=64))
    out.append(_bq("qpw", "cell", False, 65, 301, 200, 64, sm=1, a4=False, qpw=64))
    out.append(_bq("qpw", "cell", True, 32, 300, 230, 128, sm=2, a4=True, qpw=32))
    out.append(_bq("qpw", "cell", True, 33, 302, 230, 128, center=False, sm=1, a4=False, qpw=32))
    out.append(_bq("qpw", "cell", False, 32, 128, 250, 7, sm=2, a4=True, qpw=32))          # the halving loop stops at 32
    out.append(_bq("qpw", "cell", True, 1, 259, 50, 128, sm=2, a4=False, qpw=16))          # ... and runs down to 16 from 32
    out.append(_bq("qpw", "cell", True, 3, 200, 37, 7, sm=2, a4=True, qpw=16))             # ... and from 128
    # the cell-sorted pair: every build instantiation, both row formats, GROUP on and off
    for g, b, n, m, ns, build in ((True, 2, 1000, 70, 16, (1, 10, 1)), (False, 2, 1024, 37, 7, (1, 10, 1)),
                                  (True, 2, 1025, 70, 32, (4, 12, 2)), (False, 70, 1025, 37, 16, (4, 12, 2)), (True, 128, 4096, 33, 16, (4, 12, 2)),
                                  (True, 130, 1025, 40, 16, (4, 12, 1)), (False, 130, 4096, 33, 7, (4, 12, 1)),
                                  (True, 2, 4097, 70, 64, (16, 14, 4)), (False, 64, 4097, 33, 16, (16, 14, 4)), (True, 1, 16384, 70, 128, (16, 14, 4)),
                                  (True, 70, 4097, 37, 16, (16, 14, 2)), (False, 65, 4097, 33, 32, (16, 14, 2)),
                                  (True, 130, 4097, 40, 16, (16, 14, 1)), (False, 129, 4097, 33, 7, (16, 14, 1)),
                                  (True, 2, 16385, 70, 16, (0, 14, 4)), (False, 2, PACKED_MAX_N, 37, 16, (0, 14, 4)),
                                  (True, 1, PACKED_MAX_N + 1, 70, 32, (0, 14, 4)), (False, 1, PACKED_MAX_N + 1, 37, 7, (0, 14, 4))):
        out.append(_bq("build", "sorted", g, b, n, m, ns, center=ns != 32, ws=True, build=build, packed=n <= PACKED_MAX_N))
    # auto with a workspace, 32 clouds and up, more than one round of query tiles -> the sorted pair (C ABI, explicit workspace)
    out.append(_bq("auto_ws", "auto", True, 90, 300, 257, 16, ws=True, build=(1, 10, 1), packed=True))
    out.append(_bq("auto_ws", "auto", False, 32, 1100, 1025, 7, ws=True, build=(4, 12, 2), packed=True))
    # ... and just outside each condition: the cell kernel, workspace or not
    out.append(_bq("auto_ws_few_clouds", "auto", True, 31, 300, 1100, 16, ws=True, sm=1, a4=True, qpw=128))
    out.append(_bq("auto_ws_one_round", "auto", True, 128, 300, 256, 16, ws=True, sm=2, a4=True, qpw=128))
    return out


def _knn(regime, entry, b, n, m, k, **want):
    return _case("knn", regime, entry=entry, b=b, n=n, m=m, k=k, want=want)


def _knn_cases():
    out = []
    for k in KNN_SMALL_K:
        out.append(_knn("small", "all_pairs", 256, 64, 5, k))                               # 256 blocks of one ragged tile of queries
    out.append(_knn("small", "all_pairs", 128, 1030, 257, 8))                               # two data tiles (1024 + 6), two query blocks
    out.append(_knn("small", "all_pairs", 128, 64, 257, 16))
    out.append(_knn("small", "all_pairs", 256, 4096, 5, 4))                                 # the largest cloud of this kernel
    out.append(_knn("small", "all_pairs", 256, 4096, 5, 12))
    out.append(_knn("just_below_small", "all_pairs", 255, 64, 5, 8, parts=16))              # 255 blocks: the tiled kernel
    out.append(_knn("just_above_small_n", "all_pairs", 256, 4097, 5, 8, parts=16))
    out.append(_knn("parts", "all_pairs", 256, 32, 1024, 3, parts=1))                       # 262144 queries
    out.append(_knn("parts", "all_pairs", 65, 32, 1009, 3, parts=4))                        # 65585 queries, 64 per block: ragged
    out.append(_knn("parts", "all_pairs", 65, 32, 1008, 3, parts=16))                       # 65520 queries
    out.append(_knn("k_equals_n", "all_pairs", 64, 40, 1024, 40, parts=4))
    out.append(_knn("k_equals_n", "all_pairs", 3, 64, 5, 64, parts=16))
    out.append(_knn("lds_limit", "all_pairs", 2, 1500, 77, 67, parts=16))                   # the Python wrapper's largest k; two data tiles
    for k in KNN_REG_K[1:]:
        out.append(_knn("grid", "sorted", 2, 900, 300, k))
    out.append(_knn("grid", "three_nn", 2, 700, 300, 3))                                    # hf_three_nn_sorted: 700 known, 300 unknown points
    out.append(_knn("grid_any_k", "sorted", 2, 900, 300, 5))
    out.append(_knn("grid_any_k", "sorted", 1, 300, 257, 67))
    out.append(_knn("grid_limit", "sorted", 1, KNN_BIN_MAX_DATA, 20, 8))
    out.append(_knn("beyond_grid", "sorted", 1, KNN_BIN_MAX_DATA + 1, 20, 4, parts=16))     # falls back to the tiled kernel
    return out


def _topk_cases():
    return [_case("topk", "ties", b=2, m=70, n=33, k=5), _case("topk", "k_gt_n", b=1, m=300, n=7, k=9), _case("topk", "grid_loop", b=3, m=44000, n=4, k=2)]


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _fps_cases() + _bq_cases() + _knn_cases() + _topk_cases()
    return _CASES


def cases_of(family):
    return [c for c in all_cases() if c["family"] == family]


def instantiations(c):
    """the (kernel, template arguments) pairs the forced call of the case launches (the test's second, automatic call is not counted)"""
    f = c["family"]
    if f == "fps":
        d = fps_dispatch(c["n"], c["m"], c["kernel"], c["threads"])
        return {d} if d else set()
    if f == "bq":
        ws = c["ws"] or wrapper_passes_workspace(c["variant"], c["b"], c["m"])
        return set(bq_dispatch(c["variant"], c["b"], c["n"], c["m"], c["radius"], c["nsample"], c["group"], ws, not c["off"]) or ())
    if f == "knn":
        if c["entry"] == "all_pairs":
            return set(knn_dispatch(c["b"], c["n"], c["m"], c["k"]) or ())
        return set(knn_sorted_dispatch(c["b"], c["n"], c["m"], c["k"]) or ())
    return {("select_top_k_kernel", ())}


def selected_instantiations(cases=None):
    s = set()
    for c in (all_cases() if cases is None else cases):
        s |= instantiations(c)
    return s


def diagnostic_instantiations():
    return {(name, args) for name, args, _, _ in DIAGNOSTIC_ONLY}


# ---------------------------------------------------------------------------------------------- inputs
def _seed(c):
    return zlib.crc32(case_id(c).encode())


WRAP_SOURCE = 100


def wrap_block(n):
    """With the second half an exact copy of the first, the lower index of a tied pair also has the lower (k mod 512, k) at every length
    of the table, and a kernel that broke ties by index alone (or by its own wave order) would pass.  So clouds of more than 512 points
    also repeat points 100 .. 107, pushed out to four times their distance (far points are picked in the first rounds), at 512 .. 519:
    there the HIGHER index wins the tie (k mod 512 = 0 .. 7).  The slice of that block, or None."""
    return slice(FPS_TIE_MOD, FPS_TIE_MOD + min(8, n - FPS_TIE_MOD)) if n > FPS_TIE_MOD else None


def make_inputs(c):
    """float32 numpy arrays of the case"""
    rng = np.random.default_rng(_seed(c))
    f = c["family"]
    if f == "fps":
        b, n = c["b"], c["n"]
        x = (rng.normal(0, 1, (b, n, 3)) * np.array([1.5, 0.8, 2.5])).astype(np.float32)
        h, w = n // 2, wrap_block(n)
        src = slice(WRAP_SOURCE, WRAP_SOURCE + (w.stop - w.start if w else 0))
        x[:, src] *= np.float32(4)
        if w is not None and w.stop <= h:             # (inside the first half: repeated with it)
            x[:, w] = x[:, src]
        x[:, h:] = x[:, :n - h]                       # the second half repeats the first: every round has a distance tie
        if w is not None and w.stop > h:              # (in the second half: these few points repeat the block's source instead)
            x[:, w] = x[:, src]
        if c["same"] is not None:
            x[c["same"]] = x[c["same"], :1]           # one cloud of identical points: every distance is 0
        return dict(xyz=x)
    if f == "bq":
        b, n, m, r, ns = c["b"], c["n"], c["m"], np.float32(c["radius"]), c["nsample"]
        nd = min(n // 2, 2 * ns + 50)                 # a cube of side r / 2 holds nd points of every cloud: more than nsample hits each
        side = r * np.float32(max(8.0, (4.19 * n) ** (1.0 / 3.0)))    # the rest: about one hit per ball (4.19 r^3 of the box's volume per point)
        x1 = (rng.random((b, n, 3), dtype=np.float32) * side).astype(np.float32)
        dense = np.sort(rng.permutation(n)[:nd])      # spread over the index range
        x1[:, dense] = (np.array([3.3, 1.1, 5.7], np.float32) + rng.random((b, nd, 3), dtype=np.float32) * (np.float32(0.5) * r)).astype(np.float32)
        sparse = np.setdiff1d(np.arange(n), dense)
        sel = rng.integers(0, n, m)
        sel[0], sel[-1] = dense[nd // 2], sparse[len(sparse) // 2]
        sel[1], sel[2] = n - 1, 0                     # the two ends of the cloud are somebody's hit
        x2 = x1[:, sel].copy()
        x2[:, ::2] += (rng.random((b, (m + 1) // 2, 3), dtype=np.float32) - np.float32(0.5)) * (np.float32(0.2) * r)
        x2[:, 0] = x1[:, sel[0]]
        if m >= 8:
            x2[:, m // 2] += np.float32(1000)          # a query without any hit: a row of zeros
        return dict(xyz1=x1, xyz2=x2.astype(np.float32))
    if f == "knn":
        b, n, m = c["b"], c["n"], c["m"]
        side = max(3, int(round((n / 2.0) ** (1.0 / 3.0))))    # a quarter-unit lattice with about two points per site: distance ties everywhere
        x1 = (rng.integers(0, side, (b, n, 3)) * 0.25).astype(np.float32)
        if n >= 16:
            x1[:, n // 2:n // 2 + 8] = x1[:, :8]
        x2 = ((rng.integers(0, side, (b, m, 3)) + 0.5 * rng.integers(0, 2, (b, m, 3))) * 0.25).astype(np.float32)
        q = min(4, m, n)
        x2[:, :q] = x1[:, :q]
        return dict(xyz1=x1, xyz2=x2)
    return dict(dist=rng.integers(0, 6, (c["b"], c["m"], c["n"])).astype(np.float32))


# ---------------------------------------------------------------------------------------------- independent statements
def _sqdist(q, p):
    """(len(q), len(p)) fp32: (q - p)^2 summed over x, y, z from the left, every operation rounded to fp32"""
    d = q[:, None, :] - p[None, :, :]
    d = d * d
    return (d[..., 0] + d[..., 1]) + d[..., 2]


def ref_fps(xyz, m):
    """(picks (b, m) int32, tied rounds per cloud, rounds per cloud in which a tie goes to another point than the lowest index): a round
    is tied when two points share the largest running distance"""
    b, n, _ = xyz.shape
    out = np.zeros((b, m), np.int32)
    tied, higher = np.zeros(b, np.int64), np.zeros(b, np.int64)
    order = np.lexsort((np.arange(n), np.arange(n) % FPS_TIE_MOD))     # every index, by (k mod 512, k)
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    for i in range(b):
        p = xyz[i]
        td = np.full(n, 1e38, np.float32)
        old = 0
        for j in range(1, m):
            d = p - p[old]
            d = d * d
            td = np.minimum(td, (d[:, 0] + d[:, 1]) + d[:, 2])
            far = np.flatnonzero(td.astype(np.float64) == np.float64(td.max()))
            tied[i] += len(far) > 1
            old = int(far[np.argmin(rank[far])])
            higher[i] += old != far[0]
            out[i, j] = old
    return out, tied, higher


def ref_ball_query(radius, nsample, xyz1, xyz2):
    """(idx (b, m, nsample), pts_cnt (b, m), all hits per ball (b, m))"""
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    idx = np.zeros((b, m, nsample), np.int32)
    cnt = np.zeros((b, m), np.int32)
    total = np.zeros((b, m), np.int64)
    col = np.arange(nsample)[None, :]
    for i in range(b):
        hit = np.maximum(np.sqrt(_sqdist(xyz2[i], xyz1[i])), np.float32(1e-20)) < np.float32(radius)
        total[i] = hit.sum(1)
        first = np.argsort(~hit, axis=1, kind="stable")[:, :nsample]              # the hits in ascending index come first
        if first.shape[1] < nsample:
            first = np.concatenate([first, np.zeros((m, nsample - first.shape[1]), first.dtype)], axis=1)
        c = np.minimum(total[i], nsample)
        cnt[i] = c
        idx[i] = np.where(col < c[:, None], first, np.where(c[:, None] > 0, first[:, :1], 0))
    return idx, cnt, total


def ref_grouped(xyz1, xyz2, idx, center):
    g = np.take_along_axis(xyz1[:, None, :, :], idx[..., None].astype(np.int64), axis=2)
    return (g - xyz2[:, :, None, :]).astype(np.float32) if center else g


def ref_knn(k, xyz1, xyz2):
    """(val (b, m, k), idx (b, m, k), queries per cloud whose k-th place is tied): tied at the k-th place = the k-th and the (k + 1)-th
    smallest distance are equal, so the index decides who is in; with k == n (no (k + 1)-th) the (k - 1)-th and the k-th, so it decides
    the order"""
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    val = np.empty((b, m, k), np.float32)
    idx = np.empty((b, m, k), np.int32)
    tied = np.zeros(b, np.int64)
    for i in range(b):
        s = _sqdist(xyz2[i], xyz1[i])
        order = np.argsort(s.astype(np.float64), axis=1, kind="stable")            # (distance, index)
        idx[i] = order[:, :k]
        val[i] = np.take_along_axis(s, order[:, :k], axis=1)
        lo = k - 1 if k < n else k - 2
        ranked = np.take_along_axis(s, order[:, lo:lo + 2], axis=1)
        tied[i] = (ranked[:, 0] == ranked[:, 1]).sum() if ranked.shape[1] == 2 else 0
    return val, idx, tied


def ref_select_top_k(k, dist):
    """(outi, out) of the selection sort, and the rows whose first min(k, n) places hold a repeated value"""
    b, m, n = dist.shape
    out = dist.astype(np.float64).reshape(b * m, n).copy()
    outi = np.tile(np.arange(n, dtype=np.int32), (b * m, 1))
    rows = np.arange(b * m)
    for s in range(min(k, n)):
        mn = s + np.argmin(out[:, s:], axis=1)             # the first minimum of the tail
        out[rows, s], out[rows, mn] = out[rows, mn], out[rows, s].copy()
        outi[rows, s], outi[rows, mn] = outi[rows, mn], outi[rows, s].copy()
    head = np.sort(out[:, :min(k, n)], axis=1)
    tied = int((np.diff(head, axis=1) == 0).any(axis=1).sum()) if head.shape[1] > 1 else 0
    return outi.reshape(b, m, n), out.astype(np.float32).reshape(b, m, n), tied


def statement(c, t):
    """the case's outputs by the statements above, plus 'sharp': the figures the CPU test asserts on"""
    f = c["family"]
    if f == "fps":
        out, tied, higher = ref_fps(t["xyz"], c["m"])
        return dict(out=out, sharp=dict(tied_rounds=tied, higher_index_wins=higher))
    if f == "bq":
        idx, cnt, total = ref_ball_query(c["radius"], c["nsample"], t["xyz1"], t["xyz2"])
        r = dict(idx=idx, cnt=cnt, sharp=dict(fewer=int((total < c["nsample"]).sum()), more=int((total > c["nsample"]).sum()), none=int((total == 0).sum())))
        if c["group"]:
            r["grouped"] = ref_grouped(t["xyz1"], t["xyz2"], idx, c["center"])
        return r
    if f == "knn":
        val, idx, tied = ref_knn(c["k"], t["xyz1"], t["xyz2"])
        return dict(val=val, idx=idx, sharp=dict(tied_queries=tied))
    outi, out, tied = ref_select_top_k(c["k"], t["dist"])
    return dict(outi=outi, out=out, sharp=dict(tied_rows=tied))


def oracle_outputs(c, t, oracle):
    """the same outputs from the project's CPU oracle (the `oracle` package, passed in by the caller)"""
    f = c["family"]
    if f == "fps":
        return dict(out=oracle.farthest_point_sample(c["m"], t["xyz"]))
    if f == "bq":
        idx, cnt = oracle.query_ball_point(c["radius"], c["nsample"], t["xyz1"], t["xyz2"])
        r = dict(idx=idx, cnt=cnt)
        if c["group"]:
            g = oracle.group_point(t["xyz1"], idx)
            r["grouped"] = (g - t["xyz2"][:, :, None, :]).astype(np.float32) if c["center"] else g
        return r
    if f == "knn":
        if c["entry"] == "three_nn":
            val, idx = oracle.three_nn(t["xyz2"], t["xyz1"])      # (unknown, known)
        else:
            val, idx = oracle.knn_point(c["k"], t["xyz1"], t["xyz2"])
        return dict(val=val, idx=idx)
    outi, out = oracle.select_top_k(c["k"], t["dist"])
    return dict(outi=outi, out=out)
