"""Case table, restated launch rule and head layout, fp64 references and bounds of the kernel-level parity suite of the fused loss
entry points of csrc/glue.hip: hf_rpn_loss_fwd / _bwd and hf_rcnn_loss_fwd / _bwd (tests/test_loss_abi.py runs the cases on the GPU
through the C ABI, tests/test_loss_cases_cpu.py checks this module itself on any machine).  A plain helper module: nothing here imports
the library.

Launch rule, limits and layout, restated from glue.hip and include/hfops.h (NOT imported):
  threads             256 per workgroup, one row per thread and trip, rows r = block 256 + thread, then r += blocks 256
  forward             min(max(ceil(rows / 256), 1), 1024) workgroups: a thread takes a second row past 262 144 rows.  Per workgroup
                      one partial per column (RPN 4: seg, cls, reg, #fg; RCNN 5: box, bin, reg, #cls, #reg), the workspace is
                      4 bytes x columns x 1024; one more workgroup adds the partials of a column in fp64 and writes out5 / out6
  backward            min(ceil(rows / 256), 4096) workgroups: a second row past 1 048 576 rows; grad_head is zero-filled by a memset of
                      the entry point, the kernel writes the labelled class's row only; rows == 0 launches nothing
  limits              k + 1 <= 8 logits, nbx and nbt in 1..32 (register arrays of 8 and 32)
  head row            [bx nbx | rx nbx | bz nbx | rz nbx | bt nbt | rt nbt | ry | size 3], 4 nbx + 2 nbt + 4 floats, k rows per point / RoI

References (fp64 numpy, from the text of include/hfops.h, never from the kernels), per row r, with softmax p over the k + 1 logits:
  RPN   label -1: no segmentation term, no gradient, counted in rows, not foreground.  label t >= 0: p_t clipped to [1e-7, 1 - 1e-7],
        term 0.25 (1 - p_t)^2 (-log p_t); gradient d term / d p_t x p_t (delta_jt - p_j), zero where the clip is active.
        label t > 0 (foreground), on head row t - 1 and the x / z targets of class t - 1: the cross-entropy of the x, z and theta bin
        logits; smooth-L1 (0.5 d^2 below |d| = 1, |d| - 0.5 above) of the TRUE bin's residual against its target for x, z, theta, of
        y and of the three sizes.  out5 = [seg_w sum / rows, cls_w sum / max(#fg, 1), reg_w sum / max(#fg, 1), #fg, total].
  RCNN  non-empty = non_empty != 0; cls mask = (iou < cls_neg_hi or iou > cls_pos_lo) and non-empty, target 0 where iou < cls_neg_hi
        else gt_cls, a target outside 0..k is counted with no term and no gradient; reg mask = iou > reg_pos_lo and non-empty, on
        head row max(gt_cls - 1, 0); the comparisons are strict and made in float32.  out6 = [cls_w CE sum / #cls, cls_w bin CE sum
        / #reg, reg_w smooth-L1 sum / #reg, #cls, #reg, total]; a term whose count is 0 is 0.
  Both gradients are those of the total times the upstream scalar.  Every element that no formula above reaches is exactly 0.0: the
  logit gradient of an ignored or unmasked row, the head rows of the other classes, (RPN and RCNN alike) the residual slots of the
  wrong bins.  ref_rpn / ref_rcnn return those elements as the mask `live_*` == False.

Bounds, u = 2^-24, in the manner of gemm_cases.py and xconv_cases.py.
  counts      #fg, #cls, #reg are sums of 1.0f below 2^24 in fp32, then fp64: exact.
  terms       a per-row term and every gradient element go through expf and logf, whose rounding cannot be read from the code.  The
              project's rule for that (ELU_FACTOR = 4 of gemm_cases.py): 4 x the error that a plain fp32 numpy evaluation of the SAME
              reference function (ref_rpn / ref_rcnn with dt = float32) makes against its fp64 evaluation on the same inputs, measured on
              the host at run time, against the reference and never against the kernel.  The measurement is the largest error over the
              rows of the case (over the elements of a gradient array), floored at one rounding u max|ref| of the largest of them: on a
              case of a handful of rows the fp32 evaluation can equal fp64 by luck, while no fp32 result can be expected to do better
              than one rounding.  e(x) below is that number.
  forward     a column sum S = sum of n terms t_r >= 0 has one fp32 accumulator per thread over T = ceil(rows / (blocks 256)) rows, then
              eight levels of the workgroup's tree; the partials are added in fp64:
                  |dS| <= (T + 8) u sum |t_r| + n 4 e(t).
              The output is S w / divisor in fp64, rounded once: |d out| <= |dS| w / divisor + u |out|; the total is the fp64 sum of the
              three parts rounded once: the three |dS| w / divisor + u |total|.
  backward    an element is a product of the scale (weight, 1 / count, upstream: three roundings) and the per-row factor; all of it is
              in the fp32 evaluation of the reference: |d g| <= 4 e(g), one number per gradient array.  The backward reads the count from
              the out5 / out6 that the forward wrote, which is exact.  Elements outside `live_*` have the bound 0.
  clip        the focal gradient jumps to zero at p_t = 1e-7 and 1 - 1e-7, so the seeded logits keep the fp64 p_t a factor of 10 away
              from both (asserted in make_inputs); the gap-40 rows lie far beyond them (p_t < 1e-17 or 1 - p_t < 1e-16, asserted): there
              the forward term is that of the clipped value and the gradient is exactly zero.
  thresholds  the RCNN masks change an O(1) share of the outputs at an IoU equal to a threshold; the comparisons are exact in float32, so
              the reference makes them in float32 too and no tolerance is involved.
Nothing here is tuned to the device."""
import zlib

import numpy as np

from gemm_cases import ELU_FACTOR, U, cdiv  # noqa: F401

THREADS = 256
FWD_BLOCKS = 1024
BWD_BLOCKS = 4096
TREE_LEVELS = 8
MAX_K1 = 8
MAX_BINS = 32
RPN_COLUMNS, RCNN_COLUMNS = 4, 5
FWD_STRIDE = FWD_BLOCKS * THREADS           # 262 144
BWD_STRIDE = BWD_BLOCKS * THREADS           # 1 048 576

# (k, nbx, nbt) of rpn_stack_config2(), rpn_multiclass_heads(.) and RcnnConfig(); the three thresholds (cls_neg_hi, cls_pos_lo, reg_pos_lo)
# of RcnnTrainConfig(): restated, test_loss_cases_cpu.py holds them against the configurations
CONFIG_SHAPES = {"rpn_stack_config2": (1, 12, 12), "rpn_multiclass_heads": (3, 12, 12), "rcnn": (3, 6, 9)}
RCNN_THRESHOLDS = (0.45, 0.60, 0.55)
RPN_WEIGHTS = (100.0, 1.0, 1.0)             # RpnConfig: seg, cls, reg
EDGE_SHAPES = ((1, 1, 1), (1, 2, 2), (7, 32, 32), (2, 32, 1), (3, 5, 32))
BIG_SHAPE = (1, 2, 2)                       # a head row of 16 floats: the shape of every case past 262 144 rows
FWD_ROWS = (0, 1, 255, 256, 257, FWD_STRIDE, FWD_STRIDE + 1, 2 * FWD_STRIDE + 77)
BWD_ROWS = (1, 257, BWD_STRIDE, BWD_STRIDE + 1)
UPSTREAMS = (1.0, 0.37, -2.0, 0.0)
RPN_MIXES = ("background", "foreground", "ignored", "mixed", "one_fg_last", "class_k")
RCNN_MIXES = ("uniform", "thresholds", "class0", "class_outside", "empty", "non_empty_7", "below_neg_hi")
GAP = 40.0


# ---------------------------------------------------------------------------------------------- restated launch rule and layout
def fwd_blocks(rows):
    return min(max(cdiv(rows, THREADS), 1), FWD_BLOCKS)


def bwd_blocks(rows):
    return min(cdiv(rows, THREADS), BWD_BLOCKS)


def fwd_trips(rows):
    """rows per thread of the forward: the length of the fp32 chain into one accumulator"""
    return cdiv(rows, fwd_blocks(rows) * THREADS)


def bwd_trips(rows):
    return cdiv(rows, bwd_blocks(rows) * THREADS) if rows else 0


def rpn_workspace():
    return 4 * RPN_COLUMNS * FWD_BLOCKS


def rcnn_workspace():
    return 4 * RCNN_COLUMNS * FWD_BLOCKS


def limits_ok(k, nbx, nbt):
    return k > 0 and k + 1 <= MAX_K1 and 0 < nbx <= MAX_BINS and 0 < nbt <= MAX_BINS


def head_width(nbx, nbt):
    return 4 * nbx + 2 * nbt + 4


def head_groups(nbx, nbt):
    """(offset of the bin logits, bins) of x, z, theta; the residuals of a group follow its logits"""
    return (0, nbx), (2 * nbx, nbx), (4 * nbx, nbt)


def head_tail(nbx, nbt):
    """offset of ry; the three sizes follow"""
    return 4 * nbx + 2 * nbt


# ---------------------------------------------------------------------------------------------- the case table
def _case(kind, rows, shape, mix, logits="normal", upstream=1.0, off=False, weights=None, thresholds=RCNN_THRESHOLDS):
    k, nbx, nbt = shape
    assert limits_ok(k, nbx, nbt) and kind in ("rpn", "rcnn") and mix in (RPN_MIXES if kind == "rpn" else RCNN_MIXES)
    if weights is None:
        weights = RPN_WEIGHTS if kind == "rpn" else (1.0, 1.0)
    return dict(kind=kind, rows=rows, k=k, nbx=nbx, nbt=nbt, mix=mix, logits=logits, upstream=upstream, off=off, weights=tuple(weights),
                thresholds=tuple(thresholds))


def case_id(c):
    s = "%s-rows%d-k%d-nbx%d-nbt%d-%s-up%g" % (c["kind"], c["rows"], c["k"], c["nbx"], c["nbt"], c["mix"], c["upstream"])
    if c["logits"] != "normal":
        s += "-" + c["logits"]
    if c["off"]:
        s += "-off"
    return s


def all_cases():
    cfg = CONFIG_SHAPES
    e = EDGE_SHAPES
    w3, w2 = (3.0, 0.7, 1.3), (0.7, 1.3)
    rpn = [
        _case("rpn", 0, cfg["rpn_multiclass_heads"], "mixed"),
        _case("rpn", 1, e[0], "foreground"),
        _case("rpn", 1, cfg["rpn_multiclass_heads"], "background", upstream=0.37),
        _case("rpn", 255, e[2], "mixed", upstream=0.37, weights=w3),
        _case("rpn", 256, e[3], "class_k", upstream=-2.0, weights=w3),
        _case("rpn", 256, cfg["rpn_stack_config2"], "background"),
        _case("rpn", 257, e[4], "mixed", weights=w3),
        _case("rpn", 257, cfg["rpn_stack_config2"], "ignored"),
        _case("rpn", 257, cfg["rpn_stack_config2"], "foreground", upstream=0.37),
        _case("rpn", 257, cfg["rpn_multiclass_heads"], "mixed", upstream=0.0),
        _case("rpn", 300, cfg["rpn_multiclass_heads"], "mixed", logits="gap40", upstream=-2.0),
        _case("rpn", 257, e[1], "mixed", off=True, weights=w3),
        _case("rpn", FWD_STRIDE, BIG_SHAPE, "mixed"),
        _case("rpn", FWD_STRIDE + 1, BIG_SHAPE, "one_fg_last"),
        _case("rpn", 2 * FWD_STRIDE + 77, BIG_SHAPE, "mixed", upstream=0.37, weights=w3),
        _case("rpn", BWD_STRIDE, BIG_SHAPE, "mixed", upstream=-2.0),
        _case("rpn", BWD_STRIDE + 1, BIG_SHAPE, "one_fg_last"),
    ]
    rcnn = [
        _case("rcnn", 0, cfg["rcnn"], "uniform"),
        _case("rcnn", 1, e[0], "uniform"),
        _case("rcnn", 255, e[2], "uniform", upstream=0.37, weights=w2),
        _case("rcnn", 256, e[3], "uniform", upstream=-2.0, weights=w2),
        _case("rcnn", 257, e[4], "uniform", weights=w2),
        _case("rcnn", 257, cfg["rcnn"], "thresholds", weights=w2),
        _case("rcnn", 257, cfg["rcnn"], "class0", upstream=0.37),
        _case("rcnn", 257, cfg["rcnn"], "class_outside", thresholds=(0.45, 0.60, 0.75)),
        _case("rcnn", 257, cfg["rcnn"], "empty"),
        _case("rcnn", 257, cfg["rcnn"], "non_empty_7", upstream=-2.0),
        _case("rcnn", 257, cfg["rcnn"], "below_neg_hi"),
        _case("rcnn", 257, cfg["rcnn"], "uniform", upstream=0.0),
        _case("rcnn", 257, e[1], "uniform", off=True, weights=w2),
        _case("rcnn", FWD_STRIDE, BIG_SHAPE, "uniform"),
        _case("rcnn", FWD_STRIDE + 1, BIG_SHAPE, "uniform", weights=w2),
        _case("rcnn", 2 * FWD_STRIDE + 77, BIG_SHAPE, "uniform", upstream=0.37),
        _case("rcnn", BWD_STRIDE, BIG_SHAPE, "uniform", upstream=-2.0),
        _case("rcnn", BWD_STRIDE + 1, BIG_SHAPE, "uniform"),
    ]
    return rpn + rcnn


def cases_of(kind):
    return [c for c in all_cases() if c["kind"] == kind]


# ---------------------------------------------------------------------------------------------- inputs
def _softmax64(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def threshold_values(thresholds):
    """each threshold as float32 with its two float32 neighbours"""
    out = []
    for th in thresholds:
        th = np.float32(th)
        out += [np.nextafter(th, np.float32(-1)), th, np.nextafter(th, np.float32(2))]
    return np.array(out, np.float32)


def _targets(rng, rows, k, nbx, nbt):
    f = lambda *s: rng.standard_normal(s, dtype=np.float32)
    return dict(bin_x=rng.integers(0, nbx, (rows, k)).astype(np.int32), res_x=f(rows, k), bin_z=rng.integers(0, nbx, (rows, k)).astype(np.int32),
                res_z=f(rows, k), bin_theta=rng.integers(0, nbt, (rows,)).astype(np.int32), res_theta=f(rows), res_y=f(rows), res_size=f(rows, 3))


def make_inputs(c):
    """seeded by the case's id; float32 / int32 arrays under the argument names of include/hfops.h"""
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    rows, k, nbx, nbt = c["rows"], c["k"], c["nbx"], c["nbt"]
    k1, d = k + 1, head_width(nbx, nbt)
    t = _targets(rng, rows, k, nbx, nbt)
    t["head"] = rng.standard_normal((rows, k, d), dtype=np.float32)
    logits = rng.standard_normal((rows, k1), dtype=np.float32)
    if c["kind"] == "rpn":
        mix = c["mix"]
        if mix == "background":
            lab = np.zeros(rows, np.int32)
        elif mix == "foreground":
            lab = rng.integers(1, k + 1, rows).astype(np.int32)
        elif mix == "ignored":
            lab = np.full(rows, -1, np.int32)
        elif mix == "class_k":
            lab = np.full(rows, k, np.int32)
        elif mix == "one_fg_last":
            lab = np.zeros(rows, np.int32)
            lab[rows - 1:] = k
        else:       # 15 % ignored, 50 % background, the rest spread over the classes
            u = rng.random(rows)
            lab = np.where(u < 0.15, -1, np.where(u < 0.65, 0, rng.integers(1, k + 1, rows))).astype(np.int32)
        gap_up = np.zeros(rows, bool)
        gap_down = np.zeros(rows, bool)
        if c["logits"] == "gap40":          # a third of the rows each: the true logit 40 above the rest, 40 below, as drawn
            r = np.arange(rows)
            tcls = np.maximum(lab, 0)
            rest = logits.copy()
            rest[r, tcls] = np.nan
            gap_up, gap_down = r % 3 == 1, r % 3 == 2
            logits[r[gap_up], tcls[gap_up]] = np.nanmax(rest, axis=1)[gap_up] + np.float32(GAP)
            logits[r[gap_down], tcls[gap_down]] = np.nanmin(rest, axis=1)[gap_down] - np.float32(GAP)
        if rows:
            pt = _softmax64(logits)[np.arange(rows), np.maximum(lab, 0)]
            drawn = ~(gap_up | gap_down)
            assert ((pt[drawn] > 1e-6) & (pt[drawn] < 1.0 - 1e-6)).all(), "a seeded p_t within a factor of 10 of a clip point"
            assert (1.0 - pt[gap_up] < 1e-16).all() and (pt[gap_down] < 1e-17).all()
        t.update(seg_logits=logits, label=lab)
    else:
        mix = c["mix"]
        nh, pl, rl = (np.float32(v) for v in c["thresholds"])
        iou = rng.random(rows, dtype=np.float32)
        gc = rng.integers(0, k + 1, rows).astype(np.int32)
        ne = (rng.random(rows) < 0.9).astype(np.int32)
        r = np.arange(rows)
        if mix == "thresholds":
            iou = threshold_values(c["thresholds"])[r % 9]
            gc = rng.integers(1, k + 1, rows).astype(np.int32)
            ne[:] = 1
        elif mix == "class0":
            gc[:] = 0
        elif mix == "class_outside":        # between cls_pos_lo and reg_pos_lo: in the classification mask only (rows 0, 1 of 4); below
            assert pl < rl                  # cls_neg_hi the target is class 0 whatever gt_cls says (row 2 of 4)
            mid = (float(pl) + 0.02 + (float(rl) - float(pl) - 0.04) * rng.random(rows)).astype(np.float32)
            low = (float(nh) * 0.9 * rng.random(rows)).astype(np.float32)
            iou = np.where(r % 4 < 2, mid, np.where(r % 4 == 2, low, iou)).astype(np.float32)
            gc = np.where(r % 4 == 1, -1, np.where(r % 4 < 3, k + 1, gc)).astype(np.int32)
            ne[r % 4 < 3] = 1
        elif mix == "empty":
            ne[:] = 0
        elif mix == "non_empty_7":
            ne *= 7
        elif mix == "below_neg_hi":
            iou = (iou * np.float32(0.98) * nh).astype(np.float32)
            assert (iou < nh).all()
        if mix == "uniform" and rows:       # the last row in both masks, class k
            iou[-1], gc[-1], ne[-1] = 0.9, k, 1
        inside = (iou > rl) & (ne != 0)
        assert ((gc[inside] >= 0) & (gc[inside] <= k)).all(), "a class outside 0..k inside the regression mask is the caller's contract"
        t.update(cls_logits=logits, iou=iou, gt_cls=gc, non_empty=ne)
    return t


RPN_ARGS = ("seg_logits", "head", "label", "bin_x", "res_x", "bin_z", "res_z", "bin_theta", "res_theta", "res_y", "res_size")
RCNN_ARGS = ("cls_logits", "head", "iou", "gt_cls", "non_empty", "bin_x", "res_x", "bin_z", "res_z", "bin_theta", "res_theta", "res_y", "res_size")


# ---------------------------------------------------------------------------------------------- references
def _ce(v, tb):
    """cross-entropy of the rows of v against the bins tb, and the softmax, in the dtype of v"""
    r = np.arange(v.shape[0])
    m = v.max(axis=1)
    e = np.exp(v - m[:, None])
    s = e.sum(axis=1)
    return np.log(s) + m - v[r, tb], e / s[:, None]


def _smooth_l1(d):
    a = np.abs(d)
    return np.where(a < 1, a * a / 2, a - a.dtype.type(0.5))


def _smooth_l1_grad(d):
    return np.where(np.abs(d) < 1, d, np.sign(d))


def _head_rows(c, t, idx, cls0, dt, bin_scale, reg_scale):
    """the box terms of the rows idx on head row cls0: -> (cross-entropy sum of the three groups, smooth-L1 sum of the seven residuals,
    the gradient rows (n, d) with the two scales applied, their live mask)"""
    nbx, nbt = c["nbx"], c["nbt"]
    n = idx.size
    r = np.arange(n)
    h = t["head"][idx, cls0].astype(dt)
    g = np.zeros(h.shape, dt)
    live = np.zeros(h.shape, bool)
    ce_sum, reg_sum = np.zeros(n, dt), np.zeros(n, dt)
    picked = ((t["bin_x"][idx, cls0], t["res_x"][idx, cls0]), (t["bin_z"][idx, cls0], t["res_z"][idx, cls0]), (t["bin_theta"][idx], t["res_theta"][idx]))
    for (off, nb), (tb, tr) in zip(head_groups(nbx, nbt), picked):
        assert n == 0 or (tb.min() >= 0 and tb.max() < nb), "a bin target outside the bins is the caller's contract"
        ce, sm = _ce(h[:, off:off + nb], tb)
        ce_sum = ce_sum + ce
        sm[r, tb] -= 1
        g[:, off:off + nb] = sm * bin_scale
        live[:, off:off + nb] = True
        dlt = h[r, off + nb + tb] - tr.astype(dt)
        reg_sum = reg_sum + _smooth_l1(dlt)
        g[r, off + nb + tb] = _smooth_l1_grad(dlt) * reg_scale
        live[r, off + nb + tb] = True
    o = head_tail(nbx, nbt)
    dlt = h[:, o:o + 4] - np.concatenate([t["res_y"][idx, None], t["res_size"][idx]], axis=1).astype(dt)
    reg_sum = reg_sum + _smooth_l1(dlt).sum(axis=1)
    g[:, o:o + 4] = _smooth_l1_grad(dlt) * reg_scale
    live[:, o:o + 4] = True
    return ce_sum, reg_sum, g, live


def _f(dt, v):
    """a float argument of the C ABI: float32 first, then the working precision"""
    return dt(np.float32(v))


def ref_rpn(c, t, dt=np.float64):
    """-> dict: out (5), the per-row terms seg (rows with label >= 0), cls, reg (foreground rows), grad_seg (rows, k + 1), grad_head
    (rows, k, d), live_seg (rows), live_head (rows, k, d); everything evaluated in dt"""
    rows, k, nbx, nbt = c["rows"], c["k"], c["nbx"], c["nbt"]
    k1, d = k + 1, head_width(nbx, nbt)
    w_seg, w_cls, w_reg = (_f(dt, w) for w in c["weights"])
    up = _f(dt, c["upstream"])
    lab = t["label"]
    ar = np.arange(rows)
    z = t["seg_logits"].astype(dt)
    if rows:
        e = np.exp(z - z.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    else:
        p = z
    valid = lab >= 0
    tcls = np.maximum(lab, 0)
    pt_raw = p[ar, tcls]
    lo, hi = dt(1e-7), dt(1) - dt(1e-7)
    pt = np.clip(pt_raw, lo, hi)
    om = dt(1) - pt
    focal = dt(0.25) * om * om * (-np.log(pt))
    live_seg = valid & (pt_raw >= lo) & (pt_raw <= hi)
    dpt = dt(0.25) * (dt(2) * om * np.log(pt) - om * om / pt)
    onehot = (np.arange(k1)[None, :] == tcls[:, None]).astype(dt)
    grad_seg = (dpt * pt_raw)[:, None] * (onehot - p) * (w_seg / dt(max(rows, 1)) * up)
    grad_seg[~live_seg] = 0
    idx = np.nonzero(lab > 0)[0]
    nfg = idx.size
    den = dt(max(nfg, 1))
    cls0 = lab[idx] - 1
    cls, reg, g, live = _head_rows(c, t, idx, cls0, dt, w_cls / den * up, w_reg / den * up)
    grad_head = np.zeros((rows, k, d), dt)
    live_head = np.zeros((rows, k, d), bool)
    grad_head[idx, cls0] = g
    live_head[idx, cls0] = live
    seg = focal[valid]
    s64 = [float(np.sum(x.astype(np.float64))) for x in (seg, cls, reg)]
    parts = [s64[0] * float(w_seg) / max(rows, 1), s64[1] * float(w_cls) / max(nfg, 1), s64[2] * float(w_reg) / max(nfg, 1)]
    out = np.array(parts + [float(nfg), sum(parts)], np.float64)
    return dict(out=out, seg=seg, cls=cls, reg=reg, grad_seg=grad_seg, grad_head=grad_head, live_seg=live_seg, live_head=live_head, counts=(nfg,),
                divisors=(max(rows, 1), max(nfg, 1), max(nfg, 1)))


def rcnn_masks(c, t):
    """(cls mask, its target class, reg mask): strict float32 comparisons"""
    nh, pl, rl = (np.float32(v) for v in c["thresholds"])
    iou, ne = t["iou"], t["non_empty"] != 0
    assert iou.dtype == np.float32
    neg = iou < nh
    return (neg | (iou > pl)) & ne, np.where(neg, 0, t["gt_cls"]), (iou > rl) & ne


def ref_rcnn(c, t, dt=np.float64):
    """-> dict: out (6), the per-row terms box (cls-mask rows whose target is a class), bin, reg (reg-mask rows), grad_cls (rows, k + 1),
    grad_head (rows, k, d), live_cls (rows), live_head (rows, k, d); everything evaluated in dt"""
    rows, k, nbx, nbt = c["rows"], c["k"], c["nbx"], c["nbt"]
    k1, d = k + 1, head_width(nbx, nbt)
    w_cls, w_reg = (_f(dt, w) for w in c["weights"])
    up = _f(dt, c["upstream"])
    cmask, tgt, rmask = rcnn_masks(c, t)
    ncls, nreg = int(cmask.sum()), int(rmask.sum())
    live_cls = cmask & (tgt >= 0) & (tgt <= k)
    ci = np.nonzero(live_cls)[0]
    box, sm = _ce(t["cls_logits"][ci].astype(dt), tgt[ci])
    sm[np.arange(ci.size), tgt[ci]] -= 1
    grad_cls = np.zeros((rows, k1), dt)
    grad_cls[ci] = sm * (w_cls / dt(max(ncls, 1)) * up)
    idx = np.nonzero(rmask)[0]
    cls0 = np.maximum(t["gt_cls"][idx] - 1, 0)
    assert idx.size == 0 or cls0.max() < k
    den = dt(max(nreg, 1))
    bins, reg, g, live = _head_rows(c, t, idx, cls0, dt, w_cls / den * up, w_reg / den * up)
    grad_head = np.zeros((rows, k, d), dt)
    live_head = np.zeros((rows, k, d), bool)
    grad_head[idx, cls0] = g
    live_head[idx, cls0] = live
    s64 = [float(np.sum(x.astype(np.float64))) for x in (box, bins, reg)]
    parts = [s64[0] * float(w_cls) / max(ncls, 1), s64[1] * float(w_cls) / max(nreg, 1), s64[2] * float(w_reg) / max(nreg, 1)]
    out = np.array(parts + [float(ncls), float(nreg), sum(parts)], np.float64)
    return dict(out=out, box=box, bin=bins, reg=reg, grad_cls=grad_cls, grad_head=grad_head, live_cls=live_cls, live_head=live_head,
                counts=(ncls, nreg), divisors=(max(ncls, 1), max(nreg, 1), max(nreg, 1)))


REF = {"rpn": ref_rpn, "rcnn": ref_rcnn}
TERMS = {"rpn": ("seg", "cls", "reg"), "rcnn": ("box", "bin", "reg")}
OUT_NAMES = {"rpn": ("segmentation", "bin_classification", "regression", "num_foreground", "total"),
             "rcnn": ("box_classification", "bin_classification", "regression", "num_cls", "num_reg", "total")}
LOGIT_GRAD = {"rpn": "grad_seg", "rcnn": "grad_cls"}
LOGIT_LIVE = {"rpn": "live_seg", "rcnn": "live_cls"}


# ---------------------------------------------------------------------------------------------- bounds
def measured(x32, x64):
    """e(x): the largest error of the fp32 evaluation against fp64, floored at one rounding of the largest fp64 value"""
    if x64.size == 0:
        return 0.0
    assert x32.dtype == np.float32 and x64.dtype == np.float64
    return max(float(np.abs(x32.astype(np.float64) - x64).max()), U * float(np.abs(x64).max()))


def weights_of(c):
    """the weight of each of the three parts"""
    w = [float(np.float32(v)) for v in c["weights"]]
    return w if c["kind"] == "rpn" else [w[0], w[0], w[1]]


def forward_bounds(c, r64, r32):
    """-> the bound of every element of out5 / out6 (the counts: 0)"""
    trips = fwd_trips(c["rows"])
    pre = []
    for name, w, div in zip(TERMS[c["kind"]], weights_of(c), r64["divisors"]):
        t64 = r64[name]
        d_sum = (trips + TREE_LEVELS) * U * float(np.abs(t64).sum()) + t64.size * ELU_FACTOR * measured(r32[name], t64)
        pre.append(d_sum * abs(w) / div)
    out = r64["out"]
    ncount = len(r64["counts"])
    return np.array([pre[i] + U * abs(out[i]) for i in range(3)] + [0.0] * ncount + [sum(pre) + U * abs(out[-1])], np.float64)


def grad_bound(g32, g64):
    return ELU_FACTOR * measured(g32, g64)
