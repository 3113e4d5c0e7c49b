"""Cases and a NumPy restatement for csrc/eval_stats.hip (hf_proposal_stats, hf_argmax_accuracy), in the style of sampler_cases.py.

Proposal cases.  A frame is built around a GT grid (sampler_cases._gt_grid) with sampler_cases._candidate's generators: for the
GT picked as "recalled at 0.7" an 'fg' candidate (IoU >= 0.72 in fp64), for those "recalled at 0.5 only" a shifted copy whose fp64
IoU lies in (0.52, 0.68), and for the rest of the rows 'hard' candidates (around GT that are not to be recalled), 'high' ones (no
height overlap) and 'easy' ones (random boxes, mostly all-zero rows), one of them 500 m away (an all-zero row for certain:
best_gt 0).  Twin GT (gt[1] = gt[0]) force the first-argmax rule along a row, twin proposals leave two equal rows.  Padding rows
hold huge boxes that would overlap everything: they must never be read.

Conditions, asserted from the fp64 clip (sampler_cases.ref_iou3d_matrix) by check_proposal_case:
  - no column maximum over the valid proposals lies within MARGIN = 1e-3 of 0.5 or 0.7 (the fp32 kernel is within ~1e-5 of the fp64
    clip, tests/test_sampler_abi.py, so both count the same);
  - every case that CAN hold it (m >= 3 and g >= 3: a frame needs three labels and two proposals for 0 < a < b < labels) has a frame
    with 0 < recall_70 < recall_50 < labels; the cases with m = 1 or g = 1 cannot, and are checked for recall_50 in {0, 1} per label.
The seed of a case is the first of range(16) for which the conditions hold; make_proposal_inputs raises when none does.

Accuracy cases.  Logits on a grid of half-integers (many equal maxima: the first index wins), targets in -1 .. c - 1; with three
groups the first is all correct (target = argmax, or -1 where the argmax is 0), the second has nothing correct."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402

MARGIN = 1e-3
MAX_B, MAX_M, MAX_G = 1024, 512, 128
SENT_I = -7


def _fr(n, ng, r70=0, r50=0, pc=None, gc=None, twin_gt=False, twin_roi=False):
    """one frame: n valid proposals, ng labels, r70 labels recalled at 0.7, r50 more at 0.5 only; pc / gc the raw counts passed in"""
    return dict(n=n, ng=ng, r70=r70, r50=r50, pc=n if pc is None else pc, gc=ng if gc is None else gc, twin_gt=twin_gt, twin_roi=twin_roi)


def _case(name, m, g, frames):
    return dict(name=name, b=len(frames), m=m, g=g, frames=frames)


PROPOSAL_CASES = [
    _case("one_pair", 1, 1, [_fr(1, 1, r70=1)]),
    _case("one_row_no_gt", 1, 0, [_fr(1, 0)]),
    _case("m63_g3_empty_frame_between", 63, 3, [_fr(63, 3, r70=1, r50=1, twin_roi=True), _fr(40, 0), _fr(63, 2, r70=1, r50=1)]),
    _case("m64_g128_full", 64, 128, [_fr(64, 128, r70=20, r50=15)]),
    _case("m65_g128_short_counts", 65, 128, [_fr(65, 100, r70=12, r50=20), _fr(30, 5, r70=1, r50=2, twin_gt=True), _fr(65, 0)]),
    _case("m100_g3_twins", 100, 3, [_fr(100, 3, r70=1, r50=1, twin_gt=True, twin_roi=True), _fr(99, 3, r70=1, r50=1), _fr(1, 3, r70=1)]),
    _case("m100_g16_typical", 100, 16, [_fr(100, 11, r70=4, r50=3, twin_gt=True, twin_roi=True)]),
    _case("m512_g128_full", 512, 128, [_fr(512, 128, r70=50, r50=40, twin_roi=True)]),
    _case("m512_g1", 512, 1, [_fr(512, 1, r70=1), _fr(300, 1), _fr(512, 0)]),
    _case("m64_no_gt_at_all", 64, 0, [_fr(64, 0), _fr(10, 0), _fr(64, 0)]),
    _case("counts_beyond_the_padding", 65, 3, [_fr(65, 3, r70=1, r50=1, pc=70, gc=9), _fr(0, 3, pc=-2), _fr(65, 0, gc=-1)]),
]

# rows per group, groups, c
ACCURACY_CASES = [(1, 1, 2), (1, 3, 4), (63, 3, 4), (64, 1, 8), (65, 3, 2), (257, 3, 8), (257, 1, 4), (16384, 3, 4), (16384, 1, 8)]


def case_id(c):
    return c["name"] if isinstance(c, dict) else "rows%d_groups%d_c%d" % c


def can_hold_ordered_recalls(c):
    return c["m"] >= 3 and c["g"] >= 3 and any(fr["ng"] >= 3 and fr["n"] >= 2 for fr in c["frames"])


# ================================================================================================ boxes
def _mid_candidate(rng, gt):
    """a copy of the GT shifted until its fp64 3D IoU lies in (0.52, 0.68)"""
    for _ in range(2000):
        q = gt[:7].astype(np.float64) + np.concatenate([rng.normal(0, 0.3, 1), rng.normal(0, 0.05, 1), rng.normal(0, 0.15, 1), np.zeros(3),
                                                        rng.normal(0, 0.05, 1)])
        q = q.astype(np.float32)
        if 0.52 < sc.ref_iou3d(q.astype(np.float64), gt[:7].astype(np.float64)) < 0.68:
            return q
    raise sc.ConditionError("no candidate with an IoU between 0.5 and 0.7")


def _fg_candidate(rng, gt):
    for _ in range(2000):
        q = sc._candidate(rng, "fg", gt[None])
        if sc.ref_iou3d(q.astype(np.float64), gt[:7].astype(np.float64)) > 0.72:
            return q
    raise sc.ConditionError("no candidate with an IoU above 0.7")


def _hard_candidate(rng, src, gts):
    """a 'hard' candidate around one of `src` that recalls nothing: its fp64 IoU with every GT stays below 0.45"""
    for _ in range(2000):
        q = sc._candidate(rng, "hard", src)
        if sc.ref_iou3d_matrix(q[None], gts)[0].max() < 0.45:
            return q
    raise sc.ConditionError("no hard candidate below 0.45")


def _frame_boxes(rng, fr):
    """(props (n, 7), gts (ng, 8)) float32 of one frame"""
    n, ng = fr["n"], fr["ng"]
    gts = sc._gt_grid(rng, ng, False)
    if fr["twin_gt"] and ng >= 2:
        gts[1] = gts[0]
    first = 2 if fr["twin_gt"] and ng >= 2 else 0          # the twins are recalled together: keep them out of the picked sets
    order = first + rng.permutation(max(ng - first, 0))
    hit70, hit50 = order[:fr["r70"]], order[fr["r70"]:fr["r70"] + fr["r50"]]
    missed = [j for j in range(ng) if j not in set(hit70) | set(hit50)]
    rows = [_fg_candidate(rng, gts[j]) for j in hit70] + [_mid_candidate(rng, gts[j]) for j in hit50]
    if len(rows) > n:
        raise AssertionError("more recalled labels than proposals")
    kinds = ("hard", "easy", "high", "easy")
    k = 0
    while len(rows) < n:
        kind = kinds[k % len(kinds)] if ng else "easy"
        k += 1
        if kind == "hard" and not missed:
            kind = "easy"
        rows.append(_hard_candidate(rng, gts[missed], gts) if kind == "hard" else sc._candidate(rng, kind, gts))
    props = np.asarray(rows, np.float32).reshape(n, 7)
    if n > len(hit70) + len(hit50):
        props[-1, 0] += 500.0                               # far from every GT: an all-zero row
    if n:
        props = props[rng.permutation(n)]
    if fr["twin_roi"] and n >= 2:
        src = int(np.argmax(sc.ref_iou3d_matrix(props, gts)[0].max(1))) if ng else 0
        props[(src + 1) % n] = props[src]
    return props, gts


def _pack(c, boxes):
    b, m, g = c["b"], c["m"], c["g"]
    P, G = np.zeros((b, m, 7), np.float32), np.zeros((b, g, 8), np.float32)
    P[:, :, 3:6], G[:, :, 3:6], G[:, :, 7] = 1000.0, 1000.0, 2.0
    pc, gc = np.zeros(b, np.int32), np.zeros(b, np.int32)
    for f, (fr, (props, gts)) in enumerate(zip(c["frames"], boxes)):
        P[f, :len(props)], G[f, :len(gts)] = props, gts
        pc[f], gc[f] = fr["pc"], fr["gc"]
        assert min(max(fr["pc"], 0), m) == len(props) and min(max(fr["gc"], 0), g) == len(gts), (fr, m, g)
    return P, pc, G, gc


def check_proposal_case(c, mats):
    """the module docstring's conditions on the per-frame fp64 (n, ng) matrices; -> per-frame (labels, recall_50, recall_70)"""
    out, ordered = [], False
    for fr, iou in zip(c["frames"], mats):
        n, ng = iou.shape
        if n == 0 or ng == 0:
            out.append((ng, 0, 0))
            continue
        col = iou.max(axis=0)
        for thr in (0.5, 0.7):
            sc._need((np.abs(col - thr) >= MARGIN).all(), "a column maximum within %g of %g" % (MARGIN, thr))
        r50, r70 = int((col > 0.5).sum()), int((col > 0.7).sum())
        ordered = ordered or 0 < r70 < r50 < ng
        out.append((ng, r50, r70))
    if can_hold_ordered_recalls(c):
        sc._need(ordered, "no frame with 0 < recall_70 < recall_50 < labels")
    return out


_CACHE = {}


def make_proposal_inputs(c):
    """-> dict(proposals (b,m,7), proposal_count, gt (b,g,8), gt_count, mats: per-frame fp64 IoU, recalls: per-frame (labels, r50,
    r70) of the fp64 clip, data_seed); computed once per case and shared"""
    key = c["name"]
    if key in _CACHE:
        return _CACHE[key]
    last = None
    for data_seed in range(16):
        rng = np.random.default_rng(9000 + 131 * data_seed + 7 * c["m"] + c["g"])
        try:
            boxes = [_frame_boxes(rng, fr) for fr in c["frames"]]
            mats = [sc.ref_iou3d_matrix(p_, g_)[0] for p_, g_ in boxes]
            recalls = check_proposal_case(c, mats)
        except sc.ConditionError as err:
            last = err
            continue
        P, pc, G, gc = _pack(c, boxes)
        t = dict(proposals=P, proposal_count=pc, gt=G, gt_count=gc, mats=mats, recalls=recalls, data_seed=data_seed)
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = t
        return t
    raise AssertionError("%s: no seed satisfies the conditions: %s" % (key, last))


# ================================================================================================ restatement
def ref_proposal_stats(iou3d, iou2d, proposals, proposal_count, gt, gt_count):
    """box_util.compute_recall_iou per frame on given (b, m, g) matrices, plus the sums evaluator.py:1040-1064 accumulates
    -> best_iou3d, best_iou2d (b, m) in the matrices' dtype, best_gt (b, m) int32, counts (b, 4) int32, sums (b, 3) float64 (summed
    with math.fsum-like np.sum over float64 copies of the float32 values; the angle difference taken in float32)"""
    b, m, g = iou3d.shape
    best3, best2 = np.zeros((b, m), iou3d.dtype), np.zeros((b, m), iou2d.dtype)
    best_gt = np.full((b, m), -1, np.int32)
    counts, sums = np.zeros((b, 4), np.int32), np.zeros((b, 3), np.float64)
    mags = np.zeros((b, 3), np.float64)
    for f in range(b):
        n, ng = min(max(int(proposal_count[f]), 0), m), min(max(int(gt_count[f]), 0), g)
        counts[f, :2] = n, ng
        if n * ng == 0:
            continue
        m3, m2 = iou3d[f, :n, :ng], iou2d[f, :n, :ng]
        col = m3.max(axis=0)
        counts[f, 2], counts[f, 3] = (col > 0.5).sum(), (col > 0.7).sum()
        best3[f, :n], best2[f, :n] = m3.max(axis=1), m2.max(axis=1)
        am = np.argmax(m3, axis=1)
        best_gt[f, :n] = am
        ang = np.abs(proposals[f, :n, 6].astype(np.float32) - gt[f, am, 6].astype(np.float32)).astype(np.float32)
        vals = [best2[f, :n].astype(np.float64), best3[f, :n].astype(np.float64), ang.astype(np.float64)]
        sums[f] = [v.sum() for v in vals]
        mags[f] = [np.abs(v).sum() for v in vals]
    return best3, best2, best_gt, counts, sums, mags


def sum_bound(m, mags):
    """|fp64 sum of m terms in any order - the exact sum| <= (m - 1) u sum|v| (1 + O(u)) with u = 2^-53 per addition; both the
    kernel's sum and NumPy's carry it, so they differ by at most 2 (m - 1) 2^-53 sum|v| <= m 2^-52 sum|v|"""
    return m * 2.0 ** -52 * mags


def ref_argmax_accuracy(logits, target, groups):
    """calculate_cls_accuracy as counts: per group, rows whose np.argmax equals the argmax of the one-hot row of the target (all
    zero for a negative target: 0)"""
    hit = np.argmax(logits, axis=-1) == np.maximum(target, 0)
    return hit.reshape(groups, -1).sum(axis=1).astype(np.int32)


def make_accuracy_inputs(case):
    rpg, groups, c = case
    rng = np.random.default_rng(rpg * 31 + groups * 7 + c)
    rows = rpg * groups
    logits = (rng.integers(-2, 3, (rows, c)) / 2.0).astype(np.float32)
    target = rng.integers(-1, c, rows).astype(np.int32)
    am = np.argmax(logits, axis=1).astype(np.int32)
    if groups == 3:
        first = am[:rpg].copy()
        first[(first == 0) & (rng.random(rpg) < 0.5)] = -1          # a negative target is class 0
        target[:rpg] = first                                          # everything correct
        target[rpg:2 * rpg] = (am[rpg:2 * rpg] + 1) % c               # nothing correct
    return logits, target
