"""Case tables, fixtures, the fp64 reference and a model of the launch regimes of csrc/bev_iou.hip (hf_compute_bev_iou, hf_nms_mask,
hf_oriented_nms, hf_oriented_nms_batched).  Plain NumPy: the library is not imported here.

The fixture.  Boxes live on a lattice of SITES whose pitch keeps the bounding circles of different sites apart, so a pair of boxes
from two sites is an exact zero in every statement of the operation (the fp64 clip, the fp32 oracle, the device's first filter).  A
site holds g jittered copies of one box whose headings sit on distinct slots at least HEADING_SLOT rad apart inside a span below
pi/2 - HEADING_SLOT: no two members are near-parallel or near-perpendicular, which is where the reference algorithm (and its fp32
restatement, oracle/hf_oracle.c) loses its reliability.  An explicit placement -- a seeded permutation, or planted positions --
decides which index, hence which 64-box column block, every member gets.

The reference.  The IoU of a same-site pair is the fp64 Sutherland-Hodgman clip of tests/sampler_cases.py (ref_bev_overlap), taken
on the float32 box values the device reads.  `iou64 > thresh` is the adjacency; a site with a pair within MARGIN of a threshold of its
case is drawn again from the seeded generator (no box is dropped: n and the placement stay exact).  MARGIN is a provisional 1e-3;
tests/test_bev_cases_cpu.py measures the fp32 oracle's error against the fp64 clip over every same-site pair, derives the value
bound from it by the rule of sampler_cases.iou_bound (ELU_FACTOR x the largest error, floored at U) and asserts that bound + 3e-5
(the margin test_ops_gpu._drop_borderline uses) stays below MARGIN -- so the margin that holds is at least the one required.

The model.  nms_mask_kernel<true> files an entry (row i, column block c) iff some j > i in block c is adjacent to i and
c >= i // 64 + 2; nms_sweep_kernel picks its form from the per-column counts.  regime() restates that choice, flags() the
sub-regimes inside a form (ring wraps, load trips, chunks, the on-demand loop, the dense-mask gather)."""
import functools
import math
import os
import re

import numpy as np

import sampler_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(os.path.dirname(HERE), "heterofusionrcnn_amd", "csrc", "bev_iou.hip")

# ------------------------------------------------------------------------------------------------ constants of bev_iou.hip
kIouRows = 96
kIouThreads = 512
kIouStoreWaves = 2
kNmsThreads = 512
kNmsListCap = 2048
kSweepThreads = 1024
kSweepGatherers = kSweepThreads - 64
kSweepLead = 4
kStreamMaxBlocks = 1024
kStreamRing = 4096
kStreamWords = 64
kStreamMaxAverage = 32
SLAB_TILES = 65535            # grid.y limit: hf_compute_bev_iou walks taller matrices in slabs of this many row tiles
MAX_SWEEP_BLOCKS = 8192       # hf_oriented_nms refuses cb above this
CHUNK_BLOCKS = 64             # chunk_blocks = min(cb, 64): the barrier form's word pairs in LDS
STREAM_LOAD_TRIP = 64 * 4     # list entries a producer wave of the streaming sweep moves per trip
MAX_FRAMES = 65535

SENT_I = -7
HF_OK, HF_EINVAL, HF_EWORKSPACE = 0, -1, -3


def source_pins():
    """text that must stand in bev_iou.hip (compared with white space collapsed): every constant above and the literal rules"""
    return [
        "#define HF_IOU_ROWS %d" % kIouRows, "constexpr int kIouRows = HF_IOU_ROWS;",
        "#define HF_IOU_THREADS %d" % kIouThreads, "constexpr int kIouThreads = HF_IOU_THREADS;",
        "#define HF_IOU_STORE_WAVES %d" % kIouStoreWaves, "constexpr int kIouStoreWaves = HF_IOU_STORE_WAVES;",
        "#define HF_NMS_THREADS %d" % kNmsThreads, "constexpr int kNmsThreads = HF_NMS_THREADS;",
        "constexpr int kNmsListCap = %d;" % kNmsListCap,
        "constexpr int kSweepThreads = %d;" % kSweepThreads,
        "constexpr int kSweepGatherers = kSweepThreads - 64;",
        "constexpr int kSweepLead = %d;" % kSweepLead,
        "constexpr int kStreamMaxBlocks = %d;" % kStreamMaxBlocks,
        "constexpr int kStreamRing = %d;" % kStreamRing,
        "constexpr int kStreamWords = %d;" % kStreamWords,
        "constexpr int kStreamMaxAverage = %d;" % kStreamMaxAverage,
        # the slab walk of hf_compute_bev_iou
        "if (gy > %d) {" % SLAB_TILES, "for (int y0 = 0; y0 < gy; y0 += %d) {" % SLAB_TILES, "const int rows0 = y0 * kIouRows;",
        "std::min(num_a - rows0, %d * kIouRows)" % SLAB_TILES,
        # hf_oriented_nms_batched
        "if (cb > %d ||" % MAX_SWEEP_BLOCKS, "const int chunk_blocks = std::min(cb, %d);" % CHUNK_BLOCKS,
        "frames > %d" % MAX_FRAMES,
        # the filing rule of the mask kernel and the choice of the sweep's form
        "if (UPPER_ONLY && col_t > row_t + 1 && w != 0ull) {", "if (slot < kNmsListCap)",
        "if (cb <= kStreamMaxBlocks) {", "if (c > kNmsListCap) any_overflow = 1;",
        "if (mine > kStreamMaxAverage * cb / 4) any_overflow = 1;",
        "atomicAdd(&scan_ws[31], mine) + mine > kStreamMaxAverage * cb) any_overflow = 1;",
        "if (cb <= kStreamMaxBlocks && !any_overflow) {",
        # the sub-regimes
        "for (int k0 = 0; k0 < cnt; k0 += 64 * 4) {", "> kStreamRing) __builtin_amdgcn_s_sleep(2);",
        "> kStreamWords) __builtin_amdgcn_s_sleep(2);", "for (int k = u + kSweepGatherers; k < cnt; k += kSweepGatherers) {",
        "if (cnt <= kNmsListCap) {", "if (blk % chunk_blocks == 0) {",
    ]


def _collapse(text):
    return re.sub(r"\s+", " ", text)


def missing_pins(source_text):
    flat = _collapse(source_text)
    return [p for p in source_pins() if _collapse(p) not in flat]


# ------------------------------------------------------------------------------------------------ the site fixture
MIN_GAP = 1.0                 # metres left between the bounding circles of two sites (the device's filter pads them by ~1e-3)
LENGTH, WIDTH = (3.2, 4.4), (1.4, 2.0)
SIZE_JITTER = 0.10
HEADING_SLOT = 0.03           # rad: the least heading difference inside a site, and the least distance from perpendicular
HEADING_SPAN = math.pi / 2 - 2 * HEADING_SLOT - 0.004
HEADING_SLOTS = 47            # slots HEADING_SPAN / 46 = 0.0320 rad apart, each jittered by at most 0.001 rad
MARGIN = 1e-3                 # provisional (module docstring): no same-site IoU this close to a threshold of its case
MAX_REDRAWS = 200


def bev7(b):
    """(x1, y1, x2, y2, ry) float32 rows -> the (x, y, z, dx, dz, dy, ry) fp64 boxes of the same rectangles (unit height)"""
    b = np.asarray(b, np.float32).astype(np.float64).reshape(-1, 5)
    out = np.zeros((len(b), 7))
    out[:, 0], out[:, 2] = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    out[:, 3], out[:, 4] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    out[:, 1], out[:, 5], out[:, 6] = 1.0, 1.0, b[:, 4]
    return out


def ref_pair(a7, b7):
    """fp64 (overlap, iou) of two bev7 rows: the clip of sampler_cases, over max(sa + sb - overlap, 1e-8) as iou_bev does"""
    ov = sc.ref_bev_overlap(a7, b7)
    return ov, ov / max(a7[3] * a7[4] + b7[3] * b7[4] - ov, 1e-8)


def pitch_for(shift):
    """the lattice pitch at which no bounding circle of one site comes within MIN_GAP of a circle of another"""
    radius = 0.5 * (1 + SIZE_JITTER) * math.hypot(LENGTH[1], WIDTH[1])
    return math.ceil(2 * (radius + math.hypot(*shift)) + MIN_GAP)


def lattice(sites, pitch):
    """(sites, 2) centres of a square lattice centred on the origin, the innermost first.  The reference algorithm works in fp32 on
    absolute coordinates: measured with the oracle, at |x| ~ 1500 m about one overlapping pair in 10 000 loses a polygon vertex (IoU
    off by 0.02 .. 0.3), at a few hundred metres none does.  The fixtures therefore hand the innermost centres to the sites with
    the most members; singles, which take part in no overlapping pair, fill the outside."""
    w = max(1, int(math.ceil(math.sqrt(sites))))
    k = np.arange(w * w)
    xy = np.stack([(k % w - (w - 1) / 2), (k // w - (w - 1) / 2)], 1)
    order = np.argsort(np.abs(xy).max(1), kind="stable")[:sites]
    return xy[order] * pitch


def draw_site(rng, g, centre, shift):
    """g jittered copies of one box -> (g, 5) float32.  shift = (along the length, across) in metres, the largest centre offset"""
    length, width, base = rng.uniform(*LENGTH), rng.uniform(*WIDTH), rng.uniform(0, math.pi)
    if g <= HEADING_SLOTS:
        slots = rng.choice(HEADING_SLOTS, size=g, replace=False)
        head = base + slots * (HEADING_SPAN / (HEADING_SLOTS - 1)) + rng.uniform(-0.001, 0.001, g)
    else:   # more members than slots: an even step over the same span (the dense tile)
        head = base + rng.permutation(g) * (HEADING_SPAN / g)
    u, v = rng.uniform(-1, 1, g) * shift[0], rng.uniform(-1, 1, g) * shift[1]
    c, s = math.cos(base), math.sin(base)
    cx, cy = centre[0] + u * c - v * s, centre[1] + u * s + v * c
    dx = length * rng.uniform(1 - SIZE_JITTER, 1 + SIZE_JITTER, g)
    dy = width * rng.uniform(1 - SIZE_JITTER, 1 + SIZE_JITTER, g)
    return np.stack([cx - dx / 2, cy - dy / 2, cx + dx / 2, cy + dy / 2, head], 1).astype(np.float32)


def site_pairs(boxes, threshes=()):
    """fp64 (overlap, iou) of every pair a < b of a site's boxes -> (a, b, overlap, iou) arrays, or None as soon as a pair lies
    within MARGIN of one of the thresholds"""
    b7 = bev7(boxes)
    g = len(b7)
    a_i, b_i = np.triu_indices(g, 1)
    ov, iou = np.zeros(len(a_i)), np.zeros(len(a_i))
    for k, (a, b) in enumerate(zip(a_i, b_i)):
        ov[k], iou[k] = ref_pair(b7[a], b7[b])
        if any(abs(iou[k] - t) < MARGIN for t in threshes):
            return None
    return a_i, b_i, ov, iou


def make_fixture(seed, groups, positions, threshes=(), shift=(1.0, 0.5)):
    """groups: the members of every site; positions[k]: the index the k-th member (site after site) gets among the n = sum(groups)
    boxes.  -> dict(boxes (n, 5) f32, site (n,), pi, pj (final indices, pi < pj), pov, piou (fp64), redraws, shrunk)"""
    rng = np.random.default_rng(seed)
    groups = np.asarray(groups, np.int64)
    n = int(groups.sum())
    positions = np.asarray(positions, np.int64)
    assert positions.shape == (n,) and np.array_equal(np.sort(positions), np.arange(n)), "the placement is not a permutation"
    centres = np.zeros((len(groups), 2))
    centres[np.argsort(-groups, kind="stable")] = lattice(len(groups), pitch_for(shift))   # the largest sites innermost
    boxes, site = np.zeros((n, 5), np.float32), np.zeros(n, np.int64)
    pi, pj, pov, piou = [], [], [], []
    k0, redraws, shrunk = 0, 0, 0
    for s, g in enumerate(groups):
        g = int(g)
        sh, tries = shift, 0
        while True:
            b = draw_site(rng, g, centres[s], sh)
            got = site_pairs(b, threshes)
            if got is not None:
                a_i, b_i, ov, iou = got
                break
            redraws, tries = redraws + 1, tries + 1
            if tries % MAX_REDRAWS == 0:   # the margin cannot be met at this jitter: shrink it, never the margin
                sh, shrunk = (sh[0] * 0.8, sh[1] * 0.8), shrunk + 1
        pos = positions[k0:k0 + g]
        boxes[pos], site[pos] = b, s
        fa, fb = pos[a_i], pos[b_i]
        pi.append(np.minimum(fa, fb)); pj.append(np.maximum(fa, fb)); pov.append(ov); piou.append(iou)
        k0 += g
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    boxes.setflags(write=False)
    return dict(n=n, boxes=boxes, site=site, pi=cat(pi, np.int64), pj=cat(pj, np.int64), pov=cat(pov, np.float64),
                piou=cat(piou, np.float64), redraws=redraws, shrunk=shrunk, groups=groups, centres=centres, pitch=pitch_for(shift))


def split_groups(rng, n, sizes, shares):
    """site sizes drawn with the given shares until they hold n boxes exactly (the last site takes what is left)"""
    out, left = [], n
    while left > 0:
        g = min(int(rng.choice(sizes, p=shares)), left)
        out.append(g)
        left -= g
    return out


def hub_layout(seed, n, hubs, g, last_block, rest_below, others, contiguous=False, edge_pair=None):
    """`hubs` sites of g members first: the last member of hub h at index last_block * 64 + h, its other members at seeded indices in
    blocks < rest_below (contiguous: at h (g - 1) .. (h + 1)(g - 1) - 1 instead, at most one block apart, so that they file no
    entry among themselves); edge_pair: then a site of two at these two indices; then the `others` sites on the remaining indices,
    permuted -> (groups, positions)"""
    rng = np.random.default_rng(seed)
    assert hubs <= 64 and (last_block + 1) * 64 <= n and hubs * (g - 1) <= rest_below * 64
    groups = [g] * hubs + ([2] if edge_pair else []) + list(others)
    assert sum(groups) == n, (sum(groups), n)
    low = np.arange(hubs * (g - 1)) if contiguous else rng.permutation(rest_below * 64)[:hubs * (g - 1)]
    taken = np.zeros(n, bool)
    taken[low] = True
    taken[last_block * 64:last_block * 64 + hubs] = True
    if edge_pair:
        assert not taken[list(edge_pair)].any()
        taken[list(edge_pair)] = True
    rest = rng.permutation(np.flatnonzero(~taken))
    pos = []
    for h in range(hubs):
        pos.extend(low[h * (g - 1):(h + 1) * (g - 1)].tolist())
        pos.append(last_block * 64 + h)
    pos.extend(list(edge_pair or ()))
    pos.extend(rest.tolist())
    return groups, np.array(pos, np.int64)


# ------------------------------------------------------------------------------------------------ adjacency, filing, regimes
def adjacency(fx, thresh, n=None):
    """(i, j) with i < j and iou64 > thresh; n: only the pairs among the first n boxes"""
    sel = fx["piou"] > thresh
    if n is not None:
        sel &= fx["pj"] < n
    return fx["pi"][sel], fx["pj"][sel]


def filing(n, ai, aj):
    """the list counts the mask kernel files: an entry (row i, column block c) iff some j > i in block c is adjacent to i and
    c >= i // 64 + 2 -> counts (cb,)"""
    cb = (n + 63) // 64
    bj = aj // 64
    sel = bj >= ai // 64 + 2
    keys = np.unique(ai[sel] * cb + bj[sel])
    return np.bincount(keys % cb, minlength=cb)


def regime(n, counts):
    """the form nms_sweep_kernel takes"""
    cb = (n + 63) // 64
    assert len(counts) == cb
    if cb > kStreamMaxBlocks:
        return "barrier by size"
    if (counts > kNmsListCap).any():
        return "barrier by overflow"
    # a thread's share (one column each: cb <= kSweepThreads) above a quarter of the budget says "long" too
    if counts.sum() > kStreamMaxAverage * cb or (counts > kStreamMaxAverage * cb // 4).any():
        return "barrier by average"
    return "stream"


FLAGS = ("word ring wraps", "entry ring wraps", "column above 256", "column above kSweepGatherers", "second chunk",
         "overflow with chunking", "next word across chunks", "share rule alone")


def flags(n, counts, ai, aj, keep_mask):
    """the sub-regimes of the form regime() names.  keep_mask: the greedy decision per box"""
    cb = (n + 63) // 64
    r = regime(n, counts)
    out = set()
    if r == "stream":
        if cb > kStreamWords:
            out.add("word ring wraps")
        if counts.sum() > kStreamRing:
            out.add("entry ring wraps")
        if counts.max() > STREAM_LOAD_TRIP:
            out.add("column above 256")
    else:
        if cb > CHUNK_BLOCKS:
            out.add("second chunk")
            if r == "barrier by overflow":
                out.add("overflow with chunking")
            # a box kept in the last block of a chunk suppresses through its next word, which the first step of the next chunk
            # reads from memory, not from the chunk in LDS
            edge = (ai // 64 + 1 == aj // 64) & ((aj // 64) % CHUNK_BLOCKS == 0) & keep_mask[ai]
            if edge.any():
                out.add("next word across chunks")
        if ((counts > kSweepGatherers) & (counts <= kNmsListCap)).any():
            out.add("column above kSweepGatherers")
        if r == "barrier by average" and counts.sum() <= kStreamMaxAverage * cb:
            out.add("share rule alone")
    return out


def greedy_keep(n, ai, aj):
    """bev_iou.cpp:87-112 over the sparse adjacency -> (keep (n,) int32 padded with keep[0], kept, keep_mask (n,) bool)"""
    order = np.argsort(ai, kind="stable")
    ai, aj = ai[order], aj[order]
    start = np.searchsorted(ai, np.arange(n + 1))
    removed = np.zeros(n, bool)
    kept = []
    for i in range(n):
        if not removed[i]:
            kept.append(i)
            removed[aj[start[i]:start[i + 1]]] = True
    keep = np.full(n, kept[0], np.int32)
    keep[:len(kept)] = kept
    mask = np.zeros(n, bool)
    mask[kept] = True
    return keep, len(kept), mask


def chains(ai, aj, keep_mask):
    """(b, c) with b < c adjacent, b suppressed (by an earlier kept a) and c kept: greedy suppression is not transitive there.
    -> (all of them, those filed in a list: block(c) >= block(b) + 2, where the sweep's kept_row test decides)"""
    sel = ~keep_mask[ai] & keep_mask[aj]
    return int(sel.sum()), int((sel & (aj // 64 >= ai // 64 + 2)).sum())


def dense_mask(n, ai, aj):
    """hf_nms_mask's (n, cb) words from the adjacency: every tile, the bits j <= row of the diagonal tile clear"""
    cb = (n + 63) // 64
    mask = np.zeros((n, cb), np.uint64)
    for i, j in ((ai, aj), (aj, ai)):
        sel = (j // 64 != i // 64) | (j > i)
        np.bitwise_or.at(mask, (i[sel], j[sel] // 64), np.uint64(1) << (j[sel] % 64).astype(np.uint64))
    return mask


def oracle_site_error(oracle, fx):
    """the largest |fp32 oracle - fp64 clip| of the IoU over every same-site pair (site by site) -> (error, pairs)"""
    order = np.argsort(fx["site"], kind="stable")
    bounds = np.flatnonzero(np.diff(fx["site"][order])) + 1
    want = {}
    for i, j, v in zip(fx["pi"], fx["pj"], fx["piou"]):
        want[(int(i), int(j))] = v
    err = 0.0
    for idx in np.split(order, bounds):
        if len(idx) < 2:
            continue
        _, iou = oracle.compute_bev_iou(fx["boxes"][idx], fx["boxes"][idx])
        for a in range(len(idx)):
            for b in range(len(idx)):
                if idx[a] < idx[b]:
                    err = max(err, abs(float(iou[a, b]) - want[(int(idx[a]), int(idx[b]))]))
    return err, len(want)


def circles_clear(fx):
    """the smallest distance left between the bounding circles of two sites: every box lies inside the circle of radius
    (pitch - gap) / 2 around its site's centre -> gap (> 0: every cross-site pair is an exact zero in fp64 and, padded as the
    device's first filter pads it, on the device)"""
    b = fx["boxes"].astype(np.float64)
    cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
    reach = np.hypot(cx - fx["centres"][fx["site"], 0], cy - fx["centres"][fx["site"], 1]) + 0.5 * np.hypot(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])
    return fx["pitch"] - 2 * float(reach.max())


def value_bound(err):
    """the rule of sampler_cases.iou_bound"""
    return sc.ELU_FACTOR * max(err, sc.U)


# ------------------------------------------------------------------------------------------------ the NMS cases
def _perm(seed, n):
    return np.random.default_rng(seed).permutation(n)


def _hub_case(seed, n, g, others_size, contiguous):
    # a site of two across the boundary of the barrier form's chunks: box 4095 is kept (nothing precedes it in its site) and
    # suppresses box 4096 through its next word, which the first step of the second chunk reads from memory
    edge = (CHUNK_BLOCKS * 64 - 1, CHUNK_BLOCKS * 64)
    left = n - 64 * g - 2
    others = [others_size] * (left // others_size) + ([left % others_size] if left % others_size else [])
    return hub_layout(seed, n, 64, g, HUB_BLOCK, HUB_REST_BELOW, others, contiguous, edge)


HUB_BLOCK, HUB_REST_BELOW = 70, 60
LOW_SHIFT = (1.7, 0.6)        # wider centre offsets at the low thresholds: some same-site pairs must fall below 0.1 / 0.05

NMS_CASES = {
    #       n      thresholds  construction                                         regime               flags
    "B": dict(n=16384, thresh=(0.3,), regime="stream", flags={"word ring wraps", "entry ring wraps"}),
    "C": dict(n=4800, thresh=(0.1,), regime="stream", flags={"word ring wraps", "column above 256"}),
    "Cs": dict(n=4800, thresh=(0.1,), regime="barrier by average", flags={"share rule alone", "second chunk"}),
    "D": dict(n=4800, thresh=(0.1,), regime="barrier by average", flags={"second chunk", "column above kSweepGatherers"}),
    "E": dict(n=4800, thresh=(0.05,), regime="barrier by overflow", flags={"second chunk", "overflow with chunking"}),
    "F": dict(n=65600, thresh=(0.5,), regime="barrier by size", flags={"second chunk"}),
}
G_SIZES = (1, 63, 64, 65, 128, 129, 4096, 4097)
G_THRESH = (0.5, 0.0)
for _n in G_SIZES:   # at threshold 0 the two large ones hold more than kStreamMaxAverage entries per column: one chunk exactly, and one block more
    NMS_CASES["G%d" % _n] = dict(n=_n, thresh=G_THRESH, regime={0.5: "stream", 0.0: "barrier by average" if _n >= 4096 else "stream"},
                                 flags={0.5: {"word ring wraps"} if _n > 4096 else set(), 0.0: {"second chunk"} if _n > 4096 else set()})
HUB_MEMBERS = {"C": 8, "Cs": 14, "D": 22, "E": 40}
CHAIN_CASES = ("B", "C", "D", "E")


@functools.lru_cache(maxsize=None)
def nms_fixture(name):
    """the seeded fixture of an NMS case (computed once per process; callers must not modify it)"""
    c = NMS_CASES[name]
    n = c["n"]
    seed = 1000 + sorted(NMS_CASES).index(name)
    if name == "B":
        groups, pos, shift = split_groups(np.random.default_rng(seed), n, [1, 2, 3], [0.5, 0.3, 0.2]), _perm(seed + 50, n), (1.0, 0.5)
    elif name in HUB_MEMBERS:
        groups, pos = _hub_case(seed + 50, n, HUB_MEMBERS[name], 6 if name == "D" else 1, name == "Cs")
        shift = LOW_SHIFT
    elif name == "F":
        groups, pos, shift = split_groups(np.random.default_rng(seed), n, [1, 2], [0.95, 0.05]), _perm(seed + 50, n), (1.0, 0.5)
    else:
        groups, pos, shift = split_groups(np.random.default_rng(seed), n, [1, 2, 3, 4], [0.25, 0.25, 0.25, 0.25]), _perm(seed + 50, n), (1.0, 0.5)
    return make_fixture(seed + 100, groups, pos, c["thresh"], shift)


@functools.lru_cache(maxsize=None)
def nms_model(name, thresh, n=None):
    """everything the model says about a case at one of its thresholds (n: truncated to its first n boxes)"""
    fx = nms_fixture(name)
    n = fx["n"] if n is None else n
    ai, aj = adjacency(fx, thresh, n)
    counts = filing(n, ai, aj)
    keep, kept, keep_mask = greedy_keep(n, ai, aj)
    ch, ch_filed = chains(ai, aj, keep_mask)
    return dict(n=n, cb=(n + 63) // 64, thresh=thresh, ai=ai, aj=aj, counts=counts, total=int(counts.sum()), longest=int(counts.max()),
                regime=regime(n, counts), flags=flags(n, counts, ai, aj, keep_mask), keep=keep, kept=kept, keep_mask=keep_mask,
                chains=ch, chains_filed=ch_filed)


def nms_case_ids():
    return [(name, t) for name, c in NMS_CASES.items() for t in c["thresh"]]


# frames of one n whose sweeps take different forms inside one launch: C streams, D takes the barrier form, singles file nothing
BATCH_FRAMES, BATCH_THRESH = ("C", "D", "singles"), 0.1


@functools.lru_cache(maxsize=None)
def singles_fixture(n=4800):
    return make_fixture(77, [1] * n, np.arange(n), ())


def batch_frames():
    """[(boxes, model)] of the batched case"""
    out = []
    for name in BATCH_FRAMES:
        if name == "singles":
            fx = singles_fixture()
            e = np.zeros(0, np.int64)
            counts = filing(fx["n"], e, e)
            keep, kept, km = greedy_keep(fx["n"], e, e)
            out.append((fx["boxes"], dict(n=fx["n"], keep=keep, kept=kept, regime=regime(fx["n"], counts), total=0)))
        else:
            out.append((nms_fixture(name)["boxes"], nms_model(name, BATCH_THRESH)))
    return out


# ------------------------------------------------------------------------------------------------ the IoU-matrix cases
IOU_SHAPES = ((1, 1), (1, 65), (95, 1), (96, 64), (97, 63), (193, 130), (300, 3), (300, 5))
DENSE_SITE = 160
SLAB_ROWS = SLAB_TILES * kIouRows
SLAB_SHAPE = (SLAB_ROWS + 97, 3)
SLAB_PLANTED = (0, SLAB_ROWS - 1, SLAB_ROWS, SLAB_ROWS + 1, SLAB_ROWS + 96)
FAR_BOX = np.array([4998.0, 4999.0, 5002.0, 5001.0, 0.3], np.float32)   # kilometres from every site


def iou_case_ids():
    return ["%dx%d" % s for s in IOU_SHAPES] + ["dense"]


@functools.lru_cache(maxsize=None)
def iou_case(name):
    """-> dict(a (na, 5), b (nb, 5), rows, cols (the same-site pairs), ov, iou (fp64))"""
    if name == "dense":
        na, nb = kIouRows, 64
        fx = make_fixture(300, [DENSE_SITE], np.arange(DENSE_SITE), (), (0.5, 0.25))
    elif name == "slab":
        na, nb = len(SLAB_PLANTED), SLAB_SHAPE[1]
        fx = make_fixture(301, [na + nb], np.arange(na + nb), ())
    else:
        na, nb = (int(v) for v in name.split("x"))
        n = na + nb
        rng = np.random.default_rng(310 + IOU_SHAPES.index((na, nb)))
        fx = make_fixture(330 + IOU_SHAPES.index((na, nb)), split_groups(rng, n, [2, 3, 4], [0.4, 0.3, 0.3]), rng.permutation(n), ())
    sel = (fx["pi"] < na) & (fx["pj"] >= na)
    a, b = fx["boxes"][:na], fx["boxes"][na:]
    return dict(na=na, nb=nb, a=a, b=b, rows=fx["pi"][sel], cols=fx["pj"][sel] - na, ov=fx["pov"][sel], iou=fx["piou"][sel], fx=fx)


def areas(boxes):
    b = np.asarray(boxes, np.float64)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def slab_rows():
    """the (SLAB_SHAPE[0], 5) float32 rows of the slab case: FAR_BOX everywhere but on the planted rows"""
    c = iou_case("slab")
    rows = np.empty((SLAB_SHAPE[0], 5), np.float32)
    rows[:] = FAR_BOX
    rows[list(SLAB_PLANTED)] = c["a"]
    return rows


# ------------------------------------------------------------------------------------------------ the equal-heading family
# Sites of 2..6 boxes of ONE size and heading, shifted by fractions of the length (and, in the lateral variants, of the width) from
# a menu: boxes with relative shift (da L, db W) overlap in (1 - |da|)(1 - |db|) L W exactly.  Parallel edges are where the
# reference algorithm returns values far from the true overlap, so this family is compared decision by decision, and only where the
# fp32 oracle and the closed form agree.
EQUAL_SIZES = (256, 1500)
EQUAL_VARIANTS = (("rotated", True), ("rotated", False), ("aligned", True), ("aligned", False))   # (heading, lateral shift)
EQUAL_THRESH = 0.3
SHIFT_ALONG = (0.0, 0.125, 0.25, 0.375, 0.5, -0.125, -0.25, -0.375)
SHIFT_ACROSS = (0.0, 0.25, -0.25, 0.5)
EQUAL_CAP = 0.15              # the largest share of overlapping pairs on which the oracle may decide against the closed form


def equal_case_ids():
    return ["%d-%s-%s" % (n, h, "lateral" if lat else "inline") for n in EQUAL_SIZES for h, lat in EQUAL_VARIANTS]


@functools.lru_cache(maxsize=None)
def equal_case(name):
    """-> dict(boxes (n, 5) f32, pi, pj (pi < pj), piou: the closed form of every same-site pair)"""
    n, heading, lateral = name.split("-")
    n, lateral = int(n), lateral == "lateral"
    rng = np.random.default_rng(500 + equal_case_ids().index(name))
    groups = split_groups(rng, n, [2, 3, 4, 5, 6], [0.2] * 5)
    pos = rng.permutation(n)
    centres = lattice(len(groups), pitch_for((LENGTH[1] / 2, WIDTH[1] / 2)))
    menu = [(a, b) for a in SHIFT_ALONG for b in (SHIFT_ACROSS if lateral else (0.0,))]
    boxes = np.zeros((n, 5), np.float32)
    pi, pj, piou = [], [], []
    k0 = 0
    for s, g in enumerate(groups):
        length, width = rng.uniform(*LENGTH), rng.uniform(*WIDTH)
        head = rng.uniform(0.1, math.pi - 0.1) if heading == "rotated" else 0.0
        pick = [menu[k] for k in rng.choice(len(menu), size=g, replace=False)]
        c, sn = math.cos(head), math.sin(head)
        p = pos[k0:k0 + g]
        for m, (a, b) in enumerate(pick):
            # the corners are those of bev_iou's rotate_around_center: x' = dx cos + dy sin, y' = -dx sin + dy cos
            u, v = a * length, b * width
            cx, cy = centres[s][0] + u * c + v * sn, centres[s][1] - u * sn + v * c
            boxes[p[m]] = [cx - length / 2, cy - width / 2, cx + length / 2, cy + width / 2, head]
        for x in range(g):
            for y in range(x + 1, g):
                da, db = abs(pick[x][0] - pick[y][0]), abs(pick[x][1] - pick[y][1])
                o = (1 - da) * (1 - db)
                pi.append(min(p[x], p[y])); pj.append(max(p[x], p[y])); piou.append(o / (2 - o))
        k0 += g
    boxes.setflags(write=False)
    return dict(n=n, boxes=boxes, pi=np.array(pi, np.int64), pj=np.array(pj, np.int64), piou=np.array(piou))


def equal_disagreement(oracle, name):
    """pairs i < j of an equal-heading case on which the fp32 oracle and the closed form decide `iou > EQUAL_THRESH` differently
    -> (i, j, closed-form decision) of those pairs, the number of overlapping pairs, the oracle's mask"""
    c = equal_case(name)
    omask = oracle.nms_mask(c["boxes"], EQUAL_THRESH)
    bit = (omask[c["pi"], c["pj"] // 64] >> (c["pj"] % 64).astype(np.uint64)) & np.uint64(1)
    closed = c["piou"] > EQUAL_THRESH
    differ = bit.astype(bool) != closed
    return c["pi"][differ], c["pj"][differ], closed[differ], len(c["pi"]), omask
