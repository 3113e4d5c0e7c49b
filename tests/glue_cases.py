"""Case table, restated launch rule, fp32 restatements, fp64 evaluations and bounds of the kernel-level parity suite of the box codec,
the projection gather and the fusion concat of csrc/glue.hip: hf_bin_box_encode, hf_bin_box_decode, hf_bin_head_decode,
hf_project_gather, hf_project_gather_grad (the atomic form), hf_fuse_concat and hf_fuse_concat_grad (tests/test_glue_abi.py runs the
cases on the GPU through the C ABI, tests/test_glue_cases_cpu.py checks this module itself on any machine).  The loss kernels of the
same file belong to tests/loss_cases.py, hf_project_gather_grad_ordered to tests/ordered_grad_cases.py.  A plain helper module:
nothing here imports the library or torch.

Launch rule, restated from glue.hip (NOT imported; SOURCE_CONSTANTS is held against the source text by the CPU test):
  threads     256 per workgroup; grid = max(min(ceil(items / 256), kNumCU x 16 = 4096), 1) workgroups; an item index e = block 256 +
              thread, then e += grid 256: a thread takes a second item past STRIDE = 4096 x 256 = 1 048 576 items.
  items       encode: rows (one thread walks the k classes); decode, head decode: rows k; gather: b p c / VEC; atomic gradient: b p c
              (after a memset of grad_img); concat and its gradient: rows (c1 + c2) / VEC.
  VEC         gather: 4 where c % 4 == 0 and img and out are both 16-byte aligned, else 1.  concat: 4 where c1 % 4 == 0 and
              c2 % 4 == 0 and a, b and out are 16-byte aligned, else 1.  concat gradient: the same with grad_out, grad_a, grad_b, a NULL
              gradient counting as aligned; both NULL launches nothing.  The other four kernels have one form.

fp32 restatements, operation for operation from the reference's text (hf/core/bin_based_box3d_encoder.py tf_encode / tf_decode in both
ranks, the head parsing, arg-max and residual gather of hf/core/models/rpn_model.py:248-290, 593-605, 870-935, hf/core/projection.py
tf_rect_to_image with the int cast and tf.gather_nd of rpn_model.py:227-235, the path-drop concat of rpn_model.py:515-546), in
np.float32.  The library is built without contraction, and + - * /, floor, fmod, min and max are exactly rounded on both sides, so
every output that does not pass through sinf / cosf is predicted BIT FOR BIT.  tf.mod is floor-mod (np.fmod plus the sign fix).  The
Python-side constants (2 Ss - 1e-3, 2 R - 1e-3, 0.5 DELTA_THETA, 2 pi, pi, pi / 2, 3 pi / 2) are computed in double and rounded once,
as the reference's Python does before TensorFlow casts them.  Every function takes `dt`: with np.float64 the same formulas are
evaluated in double on the same fp32 inputs and constants (the fp64 evaluation).
  clip        tf.clip_by_value(x, lo, hi) with lo <= hi is restated as the library computes it, fmin(fmax(x, lo), hi) with the C rule
              that a NaN operand is ignored: equal to TensorFlow's for every ordered x; a NaN goes to lo, +inf to hi, -inf to lo.  The
              reference casts a NaN to int32 there (undefined); the library's choice keeps every bin in [0, nb), and the loss kernels
              index with it.
  int cast    tf.cast(float -> int32) truncates toward zero; a quotient that is not inside (-2^31, 2^31), NaN included, has no defined
              cast: the library stores pix = (-1, -1) for that point, which is outside every image (a zero row, as tf.gather_nd on the
              GPU gives for an index outside the map).
  cls         tf.gather_nd of the row's class; a class outside [0, k) has no row to gather: the library leaves the output row alone.

Bound of the outputs downstream of sinf / cosf (rows with a reference heading), u = 2^-24, first order:
  model       every fp32 operation adds half an ulp (relative u) of its result; sinf / cosf are within TAU = 4 ulp of the true value,
              |d sn| <= 2 TAU u |sn| (the OpenCL full-profile limit the device math library documents; not measured here).
  rotation    rx = fl(fl(cs x) + fl(sn z)):  E_rot = (2 TAU + 1) u (|cs x| + |sn z|) + |cs| E_x + |sn| E_z + u |rx|
              (E_x, E_z: what x and z already carry; rz alike with sn and cs exchanged).
  encode      x = box - ref is one rounding, E_x = u |x|;  t = rx + Ss: E_t = E_rot + u |t|;  the clip is 1-Lipschitz and exact;
              q = xs / DELTA: E_q = E_t / DELTA + u |q|;  res = (xs - (bin + 0.5) DELTA) / DELTA with the bin agreed:
              E_res = (E_t + u |(bin + 0.5) DELTA| + u |xs - (bin + 0.5) DELTA|) / DELTA + u |res|.
  decode      x = ((bin + 0.5) DELTA - Ss) + res DELTA: E_x = u (|(bin + 0.5) DELTA| + |(bin + 0.5) DELTA - Ss| + |res DELTA| + |x|);
              out = rx + ref: E = E_rot + u |out|.  The head decoder is the same after its (exact) arg-max.
  bins        a generator redraws every row whose fp64 q lies within 2 E_q of an integer (rows clamped by more than 2 E_t excepted:
              their bin is that of the clamp on both sides), so no row is left out and bins must be EQUAL everywhere.  The theta bin does
              not pass through trig: it is bit for bit.
  non-finite  a row whose offsets or heading are not finite yields a NaN or an infinite rotated offset, which the clip sends to a
              clamp: exact, compared by bits.
Nothing here is tuned to the device."""
import ctypes
import math
import zlib

import numpy as np

U = 2.0 ** -24
TAU = 4.0
THREADS = 256
NUM_CU = 256
BLOCKS_PER_CU = 16
GRID_CAP = NUM_CU * BLOCKS_PER_CU           # 4096
STRIDE = GRID_CAP * THREADS                 # 1 048 576
ALIGN = 16
LOWER_CLAMP_RCNN = 1e-3
INT_LIMIT = 2147483648.0

# (file under heterofusionrcnn_amd/csrc, regular expression with one group, the value of every match, number of matches)
SOURCE_CONSTANTS = (
    ("hf_common.h", r"constexpr int kNumCU = (\d+);", NUM_CU, 1),
    ("glue.hip", r"const long long cap = static_cast<long long>\(kNumCU\) \* (\d+);", BLOCKS_PER_CU, 1),
    ("glue.hip", r"dim3\(glue_grid\([^\n]*?, (\d+)\)\), dim3\(\d+\)", THREADS, 10),
    ("glue.hip", r"dim3\(glue_grid\([^\n]*?, \d+\)\), dim3\((\d+)\)", THREADS, 10),
    ("glue.hip", r"(?:\)|al) % (\d+) == 0", ALIGN, 4),
    ("glue.hip", r"\bc[12]? % (\d+) == 0", 4, 6),
    ("glue.hip", r"fmaxf\(dshift - r, ([0-9.e+-]+)f\)", LOWER_CLAMP_RCNN, 1),
    ("glue.hip", r"[<>] -?(\d{6,}\.\d)f", INT_LIMIT, 4),
)

KERNELS = ("project_gather_kernel", "project_gather_grad_kernel", "bin_box_decode_kernel", "bin_head_decode_kernel", "bin_box_encode_kernel",
           "fuse_concat_kernel", "fuse_concat_grad_kernel")
ENTRY = {"encode": "hf_bin_box_encode", "decode": "hf_bin_box_decode", "head": "hf_bin_head_decode", "gather": "hf_project_gather",
         "gather_grad": "hf_project_gather_grad", "concat": "hf_fuse_concat", "concat_grad": "hf_fuse_concat_grad"}


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- restated launch rule
def grid(items):
    return max(min(cdiv(items, THREADS), GRID_CAP), 1)


def trips(items):
    """items per thread of the busiest thread: 2 means the grid-stride loop is taken a second time"""
    return cdiv(items, grid(items) * THREADS)


def gather_vec(c, img_off=False, out_off=False):
    return 4 if c % 4 == 0 and not (img_off or out_off) else 1


def concat_vec(c1, c2, *offs):
    """offs: one flag per pointer (True = 4 bytes past a 16-byte boundary); a NULL gradient passes False"""
    return 4 if c1 % 4 == 0 and c2 % 4 == 0 and not any(offs) else 1


def regime(c):
    """(kernel, VEC or 0, trips) of a case by the restated rule; None: the entry point launches nothing"""
    op = c["op"]
    if op == "encode":
        return ("bin_box_encode_kernel", 0, trips(c["rows"]))
    if op == "decode":
        return ("bin_box_decode_kernel", 0, trips(c["rows"] * n_classes(c)))
    if op == "head":
        return ("bin_head_decode_kernel", 0, trips(c["rows"] * c["k"]))
    if op == "gather":
        v = gather_vec(c["c"], c["off"] == "img", c["off"] == "out")
        return ("project_gather_kernel", v, trips(c["b"] * c["p"] * c["c"] // v))
    if op == "gather_grad":
        items = c["b"] * c["p"] * c["c"]
        return ("project_gather_grad_kernel", 0, trips(items)) if items else None
    if op == "concat":
        v = concat_vec(c["c1"], c["c2"], c["off"] is not None)
        return ("fuse_concat_kernel", v, trips(c["rows"] * (c["c1"] + c["c2"]) // v))
    if op == "concat_grad":
        if c["null"] == "both":
            return None
        v = concat_vec(c["c1"], c["c2"], c["off"] is not None and c["off"] != c["null"])
        return ("fuse_concat_grad_kernel", v, trips(c["rows"] * (c["c1"] + c["c2"]) // v))
    raise KeyError(op)


def reached_instantiations(cases=None):
    """{(kernel, template arguments)} that the case table reaches"""
    out = set()
    for c in all_cases() if cases is None else cases:
        r = regime(c)
        if r:
            out.add((r[0], (r[1],) if r[1] else ()))
    return out


# ---------------------------------------------------------------------------------------------- parameter sets
def f32(x):
    """a Python-side constant: formed in double, rounded once"""
    return np.asarray(x, np.float64).astype(np.float32)


_R4 = 0.25 * math.pi
PARAMS = {
    "rpn": dict(ss=(3.0, 1.5, 1.5), deltas=(0.5, 0.25, 0.25), r=_R4, delta_theta=2 * _R4 / 12, nbt=12),          # the issue's RPN set
    "rpn_config": dict(ss=(3.0, 1.5, 1.5), deltas=(0.5, 0.25, 0.25), r=1.0 * math.pi, delta_theta=2 * (1.0 * math.pi) / 12, nbt=12),
    "rpn_k2": dict(ss=(3.0, 1.5), deltas=(0.5, 0.25), r=_R4, delta_theta=2 * _R4 / 12, nbt=12),
    "rcnn": dict(ss=(1.5, 0.75, 0.75), deltas=(0.5, 0.25, 0.25), r=_R4, delta_theta=10.0 * math.pi / 180.0, nbt=9),
    "k1": dict(ss=(2.0,), deltas=(0.5,), r=0.5, delta_theta=0.25, nbt=4),                                         # all dyadic, one class
}


def consts(name):
    p = PARAMS[name]
    ss64, d64 = np.asarray(p["ss"], np.float64), np.asarray(p["deltas"], np.float64)
    nbx = int(2 * p["ss"][0] / p["deltas"][0])
    assert all(int(2 * s / d) == nbx for s, d in zip(p["ss"], p["deltas"]))
    return dict(k=len(p["ss"]), nbx=nbx, nbt=p["nbt"], ss=f32(ss64), deltas=f32(d64), hi_xz=f32(2.0 * ss64 - 1e-3), r=np.float32(p["r"]),
                hi_theta=np.float32(2.0 * p["r"] - 1e-3), delta_theta=np.float32(p["delta_theta"]), half_delta_theta=np.float32(0.5 * p["delta_theta"]))


def n_classes(c):
    return len(PARAMS[c["params"]]["ss"])


# ---------------------------------------------------------------------------------------------- restatements
def clip(x, lo, hi):
    return np.fmin(np.fmax(x, lo), hi)


def floormod(x, y):
    """tf.mod"""
    r = np.fmod(x, y)
    return np.where((r != 0) & ((y < 0) != (r < 0)), r + y, r)


def _carry(v, dt):
    """an fp32 array or constant, carried into dt unchanged"""
    return np.asarray(v, np.float32).astype(dt)


def _rotate(th, x, z):
    """transpose(rot) [x, z] of the reference: rot = [[cos, -sin], [sin, cos]]; th broadcasts against x and z"""
    sn, cs = np.sin(th), np.cos(th)
    return cs * x + sn * z, (-sn) * x + cs * z, sn, cs


def encode(rcnn, ref_pts, ref_theta, boxes, mean_sizes, cst, dt=np.float32):
    """tf_encode -> (outputs, trace).  outputs: bin_x, res_x, bin_z, res_z (rows, k), bin_t, res_t, res_y (rows), res_size (rows, 3)"""
    with np.errstate(all="ignore"):
        ref, bx, ms = _carry(ref_pts, dt), _carry(boxes, dt), _carry(mean_sizes, dt)
        ss, deltas, hi = _carry(cst["ss"], dt), _carry(cst["deltas"], dt), _carry(cst["hi_xz"], dt)
        r, hi_t, dth, hdth = (dt(cst[n]) for n in ("r", "hi_theta", "delta_theta", "half_delta_theta"))
        rows = ref.shape[0]
        dx, dy, dz = bx[:, 0] - ref[:, 0], bx[:, 1] - ref[:, 1], bx[:, 2] - ref[:, 2]
        tr = dict(dx0=dx, dz0=dz)
        if ref_theta is not None:
            th0 = _carry(ref_theta, dt)
            dx, dz, sn, cs = _rotate(th0 * dt(-1), dx, dz)
            tr.update(sn=sn, cs=cs)
        else:
            th0 = np.zeros(rows, dt)
        tr.update(rx=dx, rz=dz)
        if not rcnn:
            pre = (bx[:, 6] - th0) + r
            dshift = clip(pre, dt(0), hi_t)
            tr.update(lo_t=dt(0))
        else:
            two_pi, pi, half_pi, three_half = (dt(np.float32(v)) for v in (2 * math.pi, math.pi, 0.5 * math.pi, 1.5 * math.pi))
            d0 = floormod(bx[:, 6] - floormod(th0, two_pi), two_pi)
            fold = (d0 > half_pi) & (d0 < three_half)
            d1 = np.where(fold, floormod(d0 + pi, two_pi), d0)
            pre = floormod(d1 + half_pi, two_pi) - r
            dshift = clip(pre, dt(np.float32(1e-3)), hi_t)
            tr.update(d0=d0, fold=fold, half_pi=half_pi, three_half=three_half, lo_t=dt(np.float32(1e-3)))
        tr.update(pre_t=pre, hi_t=hi_t, th0=th0)
        out = {}
        for n, d in (("x", dx), ("z", dz)):
            t = d[:, None] + ss[None, :]
            xs = clip(t, dt(0), hi[None, :])
            q = xs / deltas
            f = np.floor(q)
            centre = (f + dt(0.5)) * deltas
            out["bin_" + n] = f.astype(np.int32)
            out["res_" + n] = (xs - centre) / deltas
            tr.update({"t" + n: t, "s" + n: xs, "q" + n: q, "centre_" + n: centre})
        ft = np.floor(dshift / dth)
        out["bin_t"] = ft.astype(np.int32)
        out["res_t"] = (dshift - (ft + dt(0.5)) * dth) / hdth
        out["res_y"] = dy
        out["res_size"] = (bx[:, 3:6] - ms) / ms
    return out, tr


ENCODE_OUT = ("bin_x", "res_x", "bin_z", "res_z", "bin_t", "res_t", "res_y", "res_size")
ENCODE_TRIG = ("bin_x", "res_x", "bin_z", "res_z")          # downstream of sinf / cosf where a heading tensor is given


def rotation_bound(cs, sn, x, z, ex, ez, out):
    return (2 * TAU + 1) * U * (np.abs(cs * x) + np.abs(sn * z)) + np.abs(cs) * ex + np.abs(sn) * ez + U * np.abs(out)


def encode_bounds(o64, t64, cst):
    """from the fp64 evaluation of a case with a heading tensor: {"q_x", "res_x", "t_x", ...} (rows, k)"""
    deltas = cst["deltas"].astype(np.float64)
    ex, ez = U * np.abs(t64["dx0"]), U * np.abs(t64["dz0"])
    e_rot = dict(x=rotation_bound(t64["cs"], t64["sn"], t64["dx0"], t64["dz0"], ex, ez, t64["rx"]),
                 z=rotation_bound(t64["sn"], t64["cs"], t64["dx0"], t64["dz0"], ex, ez, t64["rz"]))
    b = {}
    for n in ("x", "z"):
        e_t = e_rot[n][:, None] + U * np.abs(t64["t" + n])
        b["t_" + n] = e_t
        b["q_" + n] = e_t / deltas + U * np.abs(t64["q" + n])
        b["res_" + n] = (e_t + U * np.abs(t64["centre_" + n]) + U * np.abs(t64["s" + n] - t64["centre_" + n])) / deltas + U * np.abs(o64["res_" + n])
    return b


def undecided_bins(o64, t64, cst):
    """(rows) True where the x or z bin of some class could differ between two evaluations inside the bound"""
    b = encode_bounds(o64, t64, cst)
    hi = cst["hi_xz"].astype(np.float64)
    bad = np.zeros(t64["rx"].shape[0], bool)
    for n in ("x", "z"):
        q, t, e_t = t64["q" + n], t64["t" + n], b["t_" + n]
        near = np.abs(q - np.rint(q)) <= 2 * b["q_" + n]
        deep = (t < -2 * e_t) | (t > hi[None, :] + 2 * e_t)
        bad |= (near & ~deep).any(axis=1)
    return bad


def decode(ref_pts, ref_theta, bin_x, res_x, bin_z, res_z, bin_t, res_t, res_y, res_size, mean_sizes, cst, dt=np.float32):
    """tf_decode -> (boxes (rows, k, 7), trace); per (row, class) inputs (rows, k[, 3])"""
    ref, ss, deltas = _carry(ref_pts, dt), _carry(cst["ss"], dt), _carry(cst["deltas"], dt)
    r, dth = dt(cst["r"]), dt(cst["delta_theta"])
    rx_, rz_, rt_, ry_, rs_, ms = (_carry(v, dt) for v in (res_x, res_z, res_t, res_y, res_size, mean_sizes))
    ax, az = (bin_x.astype(dt) + dt(0.5)) * deltas, (bin_z.astype(dt) + dt(0.5)) * deltas
    dx = ax - ss + rx_ * deltas
    dz = az - ss + rz_ * deltas
    tr = dict(dx0=dx, dz0=dz, e_dx0=U * (np.abs(ax) + np.abs(ax - ss) + np.abs(rx_ * deltas) + np.abs(dx)),
              e_dz0=U * (np.abs(az) + np.abs(az - ss) + np.abs(rz_ * deltas) + np.abs(dz)))
    if ref_theta is not None:
        th0 = _carry(ref_theta, dt)[:, None]
        dx, dz, sn, cs = _rotate(th0, dx, dz)
        tr.update(sn=sn, cs=cs)
    else:
        th0 = np.zeros((ref.shape[0], 1), dt)
    tr.update(rx=dx, rz=dz)
    boxes = np.empty(bin_x.shape + (7,), dt)
    boxes[..., 0] = dx + ref[:, None, 0]
    boxes[..., 1] = ry_ + ref[:, None, 1]
    boxes[..., 2] = dz + ref[:, None, 2]
    boxes[..., 3:6] = ms + rs_ * ms
    boxes[..., 6] = th0 + (bin_t.astype(dt) + dt(0.5)) * dth - r + rt_ * dt(0.5) * dth
    return boxes, tr


DECODE_TRIG = (0, 2)                                       # box columns downstream of sinf / cosf where a heading tensor is given


def decode_bounds(b64, t64):
    """(rows, k, 7): the bound of columns 0 and 2 of a case with a heading tensor, 0 elsewhere (those are bit for bit)"""
    e = np.zeros(b64.shape)
    e[..., 0] = rotation_bound(t64["cs"], t64["sn"], t64["dx0"], t64["dz0"], t64["e_dx0"], t64["e_dz0"], t64["rx"]) + U * np.abs(b64[..., 0])
    e[..., 2] = rotation_bound(t64["sn"], t64["cs"], t64["dx0"], t64["dz0"], t64["e_dx0"], t64["e_dz0"], t64["rz"]) + U * np.abs(b64[..., 2])
    return e


def head_width(nbx, nbz, nbt):
    return 2 * nbx + 2 * nbz + 2 * nbt + 4


def parse_head(head, nbx, nbz, nbt):
    """_parse_rpn_output: the eight slices of the last axis"""
    edges = np.cumsum([0, nbx, nbx, nbz, nbz, nbt, nbt, 1, 3])
    assert edges[-1] == head.shape[-1]
    return [head[..., a:b] for a, b in zip(edges[:-1], edges[1:])]


def head_decode(head, ref_pts, ref_theta, mean_sizes_k, nbx, nbz, nbt, cst, cls=None, dt=np.float32):
    """head (rows, k, d) -> (boxes, trace, bins): boxes (rows, k, 7), or with cls (rows, 7) and the mask of the rows that are written;
    tf.argmax takes the first maximum, the residual is that of the winning bin"""
    lx, rx, lz, rz, lt, rt, ry, rs = parse_head(head, nbx, nbz, nbt)
    pick = lambda res, b: np.take_along_axis(res, b[..., None], axis=-1)[..., 0]
    bx, bz, bt = (np.argmax(v, axis=-1).astype(np.int32) for v in (lx, lz, lt))
    rows, k = head.shape[:2]
    ms = np.broadcast_to(np.asarray(mean_sizes_k, np.float32)[None], (rows, k, 3))
    boxes, tr = decode(ref_pts, ref_theta, bx, pick(rx, bx), bz, pick(rz, bz), bt, pick(rt, bt), ry[..., 0], rs, ms, cst, dt)
    return boxes, tr, (bx, bz, bt)


def gather_cls(boxes, cls, fill=np.nan):
    """(rows, k, 7), cls (rows) -> (rows, 7) and the mask of valid rows; the others hold `fill`"""
    k = boxes.shape[1]
    valid = (cls >= 0) & (cls < k)
    out = np.full((boxes.shape[0], 7), fill, boxes.dtype)
    out[valid] = boxes[np.nonzero(valid)[0], cls[valid]]
    return out, valid


def project(pts, calib, dt=np.float32):
    """tf_rect_to_image + tf.cast(int32): pts (b, p, 3), calib (b, 12) -> (pix (b, p, 2) int32 [u, v], uf, vf)"""
    with np.errstate(all="ignore"):
        P = _carry(calib, dt)[:, None, :]
        x, y, z = (_carry(pts, dt)[..., i] for i in range(3))
        row = lambda i: P[..., 4 * i] * x + P[..., 4 * i + 1] * y + P[..., 4 * i + 2] * z + P[..., 4 * i + 3]
        d = row(2)
        uf, vf = row(0) / d, row(1) / d
        lim = dt(INT_LIMIT)
        ok = (uf > -lim) & (uf < lim) & (vf > -lim) & (vf < lim)
        pix = np.stack([np.trunc(np.where(ok, uf, -1)), np.trunc(np.where(ok, vf, -1))], axis=-1).astype(np.int64).astype(np.int32)
    return pix, uf, vf


def inside(pix, h, w):
    return (pix[..., 0] >= 0) & (pix[..., 0] < w) & (pix[..., 1] >= 0) & (pix[..., 1] < h)


def gather(img, pix):
    """tf.gather_nd(img, [b, v, u]); a pixel outside the map gives a zero row"""
    b, h, w, c = img.shape
    ok = inside(pix, h, w)
    u, v = np.where(ok, pix[..., 0], 0), np.where(ok, pix[..., 1], 0)
    out = img[np.arange(b)[:, None], v, u]
    return np.where(ok[..., None], out, np.float32(0))


def gather_grad(grad_out, pix, b, h, w, c):
    """the fp64 scatter, rounded once"""
    g = np.zeros((b, h, w, c), np.float64)
    if grad_out.size:
        ok = inside(pix, h, w)
        bi = np.broadcast_to(np.arange(b)[:, None], ok.shape)
        np.add.at(g, (bi[ok], pix[..., 1][ok], pix[..., 0][ok]), grad_out.astype(np.float64)[ok])
    return g.astype(np.float32)


MASKS = {"null": None, "pc_only": (1.0, 0.0), "img_only": (0.0, 1.0), "scaled": (0.5, 2.0)}


def concat(a, b, masks):
    m0, m1 = (np.float32(1), np.float32(1)) if masks is None else (np.float32(masks[0]), np.float32(masks[1]))
    return np.concatenate([a * m0, b * m1], axis=1)


def concat_grad(g, c1, masks):
    m0, m1 = (np.float32(1), np.float32(1)) if masks is None else (np.float32(masks[0]), np.float32(masks[1]))
    return g[:, :c1] * m0, g[:, c1:] * m1


# ---------------------------------------------------------------------------------------------- the case table
SMALL_ROWS = 300                                            # 900 items at k = 3: more than one workgroup, a ragged last one
TRIP2_ROWS_K1 = STRIDE + 77                                 # encode: items = rows
TRIP2_ROWS_K3 = (STRIDE + 17) // 3                          # decoders: 349 531 rows x 3 = STRIDE + 17
TRIP2_GATHER_V4 = (2, 524307, 4)                            # b, p, c: b p c / 4 = STRIDE + 38
TRIP2_GATHER_V1 = (2, 174770, 3)                            # b p c = STRIDE + 44
TRIP2_CONCAT_ROWS = 524297                                  # (4, 4) / 4 and (1, 1): rows x 2 = STRIDE + 18
assert TRIP2_ROWS_K3 * 3 == STRIDE + 17

ENCODE_FAMILIES = ("dyadic", "background", "random", "nonfinite")
HEADINGS = ("none", "zero", "random")


def _encode(params, rcnn, family, heading="none", rows=None, off=False, expect_trips=1):
    assert family in ENCODE_FAMILIES and heading in HEADINGS
    if rows is None:
        rows = {"dyadic": 641, "background": 1000, "random": 2000, "nonfinite": 3 * 33}[family]
    return dict(op="encode", params=params, rcnn=rcnn, family=family, heading=heading, rows=rows, off=off,
                expect=("bin_box_encode_kernel", 0, expect_trips))


def _decode(params, heading="none", rows=SMALL_ROWS, off=False, expect_trips=1):
    return dict(op="decode", params=params, heading=heading, rows=rows, off=off, expect=("bin_box_decode_kernel", 0, expect_trips))


def _head(params, bins, heading="none", cls=False, rows=SMALL_ROWS, k=None, off=False, expect_trips=1):
    return dict(op="head", params=params, k=k or len(PARAMS[params]["ss"]), bins=bins, heading=heading, cls=cls, rows=rows, off=off,
                expect=("bin_head_decode_kernel", 0, expect_trips))


def _gather(family, b, p, h, w, c, off=None, pix=True, expect_vec=None, expect_trips=1):
    assert family in ("exact", "general", "tiles") and off in (None, "img", "out")
    return dict(op="gather", family=family, b=b, p=p, h=h, w=w, c=c, off=off, pix=pix, expect=("project_gather_kernel", expect_vec, expect_trips))


def _gather_grad(b, p, h, w, c, off=False, expect_trips=1):
    return dict(op="gather_grad", b=b, p=p, h=h, w=w, c=c, off=off, expect=("project_gather_grad_kernel", 0, expect_trips) if p else None)


def _concat(op, rows, c1, c2, masks, off=None, null=None, expect_vec=None, expect_trips=1):
    assert masks in MASKS and op in ("concat", "concat_grad")
    names = ("a", "b", "out") if op == "concat" else ("grad_out", "grad_a", "grad_b")
    assert off is None or off in names
    kern = "fuse_concat_kernel" if op == "concat" else "fuse_concat_grad_kernel"
    return dict(op=op, rows=rows, c1=c1, c2=c2, masks=masks, off=off, null=null, expect=None if null == "both" else (kern, expect_vec, expect_trips))


CONCAT_SHAPES = ((4, 4), (256, 32), (5, 3), (4, 3), (3, 4), (1, 1))
GATHER_CHANNELS = (1, 3, 4, 8, 32)
HEAD_BINS = ((12, 12, 12), (6, 6, 9), (5, 7, 3), (1, 1, 1))


def all_cases():
    cs = []
    # ---- encode: the dyadic edge family (no trig: every intermediate is an exact fp32 number), both ranks, every parameter set
    cs += [_encode("rpn", 0, "dyadic"), _encode("rpn_config", 0, "dyadic"), _encode("rcnn", 1, "dyadic"), _encode("k1", 0, "dyadic"), _encode("k1", 1, "dyadic"),
           _encode("rpn", 0, "dyadic", "zero"), _encode("rcnn", 1, "dyadic", "zero")]
    # the background rows of rpn_targets: all-zero boxes against far points
    cs += [_encode("rpn", 0, "background"), _encode("rpn_config", 0, "background")]
    # seeded rows without and with a heading tensor (the second: x / z by the bound, bins equal after the redraw)
    cs += [_encode("rpn", 0, "random"), _encode("rcnn", 1, "random"), _encode("rpn", 0, "random", "random"), _encode("rpn_config", 0, "random", "random"),
           _encode("rcnn", 1, "random", "random"), _encode("k1", 1, "random", "random"), _encode("rcnn", 1, "random", "random", off=True),
           _encode("rpn", 0, "random", "zero"), _encode("rcnn", 1, "random", "zero")]
    cs += [_encode("rpn", 0, "nonfinite"), _encode("rcnn", 1, "nonfinite"), _encode("rpn", 0, "nonfinite", "random"), _encode("rcnn", 1, "nonfinite", "random")]
    cs += [_encode("k1", 0, "random", rows=TRIP2_ROWS_K1, expect_trips=2)]
    # ---- decode
    cs += [_decode("rpn"), _decode("rcnn", "random"), _decode("k1"), _decode("k1", "random"), _decode("rpn_k2", "random"), _decode("rpn_k2"),
           _decode("rpn", "zero"), _decode("rcnn", "zero"), _decode("rcnn", "random", off=True), _decode("rpn", rows=TRIP2_ROWS_K3, expect_trips=2)]
    # ---- head decode: the bin counts of both stages, three different counts, one bin per slice; with and without cls
    cs += [_head("rpn", (12, 12, 12)), _head("rpn", (12, 12, 12), cls=True), _head("rcnn", (6, 6, 9), "random"), _head("rcnn", (6, 6, 9), "random", cls=True),
           _head("rpn_k2", (5, 7, 3)), _head("rpn_k2", (5, 7, 3), "random", cls=True), _head("rpn", (5, 7, 3), cls=True), _head("k1", (1, 1, 1)),
           _head("k1", (1, 1, 1), "random", cls=True), _head("rpn", (1, 1, 1), cls=True), _head("rpn", (1, 1, 1), cls=True, rows=3), _head("rcnn", (6, 6, 9), "zero"),
           _head("rcnn", (6, 6, 9), "zero", cls=True), _head("rcnn", (6, 6, 9), "random", off=True),
           _head("rpn", (1, 1, 1), rows=TRIP2_ROWS_K3, expect_trips=2)]
    # ---- projection gather
    for c in GATHER_CHANNELS:
        cs.append(_gather("exact", 2, 96, 6, 10, c, expect_vec=4 if c % 4 == 0 else 1))
    cs += [_gather("exact", 2, 96, 6, 10, 4, off="img", expect_vec=1), _gather("exact", 2, 96, 6, 10, 8, off="out", expect_vec=1),
           _gather("exact", 2, 96, 6, 10, 4, pix=False, expect_vec=4), _gather("exact", 2, 96, 6, 10, 3, pix=False, expect_vec=1),
           _gather("general", 2, 500, 12, 40, 4, expect_vec=4), _gather("general", 2, 500, 12, 40, 3, expect_vec=1),
           _gather("general", 2, 500, 12, 40, 32, off="img", expect_vec=1),
           _gather("tiles", *TRIP2_GATHER_V4[:2], 3, 5, TRIP2_GATHER_V4[2], expect_vec=4, expect_trips=2),
           _gather("tiles", *TRIP2_GATHER_V1[:2], 3, 5, TRIP2_GATHER_V1[2], expect_vec=1, expect_trips=2)]
    cs += [_gather_grad(2, 300, 3, 5, 1), _gather_grad(2, 300, 3, 5, 4), _gather_grad(2, 300, 3, 5, 5, off=True), _gather_grad(2, 0, 3, 5, 4),
           _gather_grad(*TRIP2_GATHER_V1[:2], 3, 5, TRIP2_GATHER_V1[2], expect_trips=2)]
    # ---- fusion concat and its gradient
    names = list(MASKS)
    for op, bufs in (("concat", ("a", "b", "out")), ("concat_grad", ("grad_out", "grad_a", "grad_b"))):
        for i, (c1, c2) in enumerate(CONCAT_SHAPES):
            cs.append(_concat(op, SMALL_ROWS, c1, c2, names[i % 4], expect_vec=4 if c1 % 4 == 0 and c2 % 4 == 0 else 1))
        cs += [_concat(op, SMALL_ROWS, 4, 4, m, expect_vec=4) for m in names[1:]]
        cs += [_concat(op, SMALL_ROWS, 5, 3, "scaled", expect_vec=1)]
        cs += [_concat(op, SMALL_ROWS, 4, 4, "scaled", off=o, expect_vec=1) for o in bufs]
        cs += [_concat(op, TRIP2_CONCAT_ROWS, 4, 4, "scaled", expect_vec=4, expect_trips=2),
               _concat(op, TRIP2_CONCAT_ROWS, 1, 1, "scaled", expect_vec=1, expect_trips=2)]
    for null in ("grad_a", "grad_b", "both"):
        cs += [_concat("concat_grad", SMALL_ROWS, 4, 4, "scaled", null=null, expect_vec=4), _concat("concat_grad", SMALL_ROWS, 5, 3, "scaled", null=null, expect_vec=1)]
    # a misaligned pointer that is not passed (NULL) does not count; a misaligned one that is passed does
    cs += [_concat("concat_grad", SMALL_ROWS, 4, 4, "scaled", off="grad_b", null="grad_a", expect_vec=1)]
    return cs


def case_id(c):
    skip = ("op", "expect")
    parts = [c["op"]]
    for key, v in c.items():
        if key in skip or v is None or v is False:
            continue
        if key == "bins":
            v = "x".join(str(n) for n in v)
        parts.append("%s" % key if v is True else "%s=%s" % (key, v))
    return "-".join(parts)


def cases_of(op):
    return [c for c in all_cases() if c["op"] == op]


# ---------------------------------------------------------------------------------------------- generators
def rng_of(c, salt=0):
    return np.random.default_rng(zlib.crc32(case_id(c).encode()) + salt)


def grid64(g, lo, hi, size):
    """multiples of 1 / 64 in [lo, hi]"""
    return (g.integers(int(lo * 64), int(hi * 64) + 1, size=size) / 64.0).astype(np.float32)


def theta_specials(cst, rcnn):
    """box headings against a reference heading of 0: every clamp, both ends, every interior edge (RPN rank); every fold branch, the two
    strict comparisons and both clamps (RCNN rank)"""
    r, dth = np.float32(cst["r"]), np.float32(cst["delta_theta"])
    nxt = lambda v, to: np.nextafter(np.float32(v), np.float32(to), dtype=np.float32)
    if not rcnn:
        hi = np.float32(cst["hi_theta"])
        v = [-r - np.float32(1), nxt(-r, -9), -r, nxt(-r, 9), np.float32(0), hi - r, nxt(hi - r, 9), nxt(hi - r, -9), r, nxt(r, 9), r + np.float32(1)]
        v += [np.float32(n) * dth - r for n in range(1, cst["nbt"])]
        return np.array(v, np.float32)
    hp, thp, two_pi, pi = (np.float32(x) for x in (0.5 * math.pi, 1.5 * math.pi, 2 * math.pi, math.pi))
    v = [hp, nxt(hp, 9), nxt(hp, -9), thp, nxt(thp, 9), nxt(thp, -9), 0.0, pi, two_pi, nxt(two_pi, 0), -0.1, 7.0, -7.0, 5.0, 1.5, 0.3, 1.0, 2.0, 4.0, 6.0, -3.0,
         r + hp, 0.8, 5.6]
    return np.array(v, np.float32)


NONFINITE = (np.nan, np.inf, -np.inf)


def encode_inputs(c):
    """-> dict(ref_pts (rows, 3), ref_theta (rows) or None, boxes (rows, 7), mean_sizes (rows, 3), cst, redraws)"""
    cst = consts(c["params"])
    g = rng_of(c)
    rows, fam, rcnn = c["rows"], c["family"], c["rcnn"]
    s0 = float(cst["ss"][0])
    ms = g.uniform(0.5, 4.0, (rows, 3)).astype(np.float32)
    size = (ms * g.uniform(0.7, 1.3, (rows, 3))).astype(np.float32)
    ref_theta, redraws = None, 0

    def draw(n):
        ref = np.stack([g.uniform(-40, 40, n), g.uniform(-2, 3, n), g.uniform(0, 70, n)], axis=1).astype(np.float32)
        off = g.uniform(-1.4 * s0, 1.4 * s0, (n, 3))
        off[:, 1] = g.uniform(-1, 1, n)
        th0 = g.uniform(-7, 7, n).astype(np.float32) if rcnn else g.uniform(-math.pi, math.pi, n).astype(np.float32)
        span = 7.0 if rcnn else 1.3 * float(cst["r"])
        return ref, (ref + off).astype(np.float32), th0, g.uniform(-span, span, n).astype(np.float32)

    if fam == "dyadic":
        sweep = (np.arange(-320, 321) / 64.0).astype(np.float32)       # every multiple of 1 / 64 in [-5, 5]: all edges of all classes
        assert rows == sweep.size
        ref = np.stack([grid64(g, -40, 40, rows), grid64(g, -2, 3, rows), grid64(g, 0, 70, rows)], axis=1)
        xyz = np.stack([ref[:, 0] + sweep, ref[:, 1] + grid64(g, -1, 1, rows), ref[:, 2] + np.roll(sweep[::-1], 97)], axis=1)
        spec = theta_specials(cst, rcnn)
        heading = spec[np.arange(rows) % spec.size]
    elif fam == "background":
        ref, _, _, _ = draw(rows)
        xyz, heading, size = np.zeros((rows, 3), np.float32), np.zeros(rows, np.float32), np.zeros((rows, 3), np.float32)
    else:
        ref, xyz, th0, dh = draw(rows)
        heading = dh if c["heading"] != "random" else (th0 + dh).astype(np.float32)
        if c["heading"] == "random":
            ref_theta = th0
    boxes = np.concatenate([xyz, size, heading[:, None]], axis=1).astype(np.float32)
    if c["heading"] == "zero":
        ref_theta = np.zeros(rows, np.float32)
    if fam == "nonfinite":
        # row 3 f + v: field f (box 0..6, ref 7..9, heading 10) holds value v; three more rows with two fields at once
        for f in range(11):
            for vi, v in enumerate(NONFINITE):
                i = 3 * f + vi
                if f < 7:
                    boxes[i, f] = v
                elif f < 10:
                    ref[i, f - 7] = v
                elif ref_theta is not None:
                    ref_theta[i] = v
        if ref_theta is not None:
            ref_theta[:33] = np.where(np.isfinite(ref_theta[:33]), np.array([0.5, 2.0, -2.5], np.float32)[np.arange(33) % 3], ref_theta[:33])
    if ref_theta is not None and c["heading"] == "random":
        # redraw the rows whose x / z bin is not decided inside the bound; no row is dropped
        for _ in range(40):
            o64, t64 = encode(rcnn, ref, ref_theta, boxes, ms, cst, np.float64)
            finite = np.isfinite(t64["rx"]) & np.isfinite(t64["rz"])
            with np.errstate(invalid="ignore"):
                bad = undecided_bins(o64, t64, cst) & finite
            if not bad.any():
                break
            n = int(bad.sum())
            redraws += n
            r2, x2, t2, d2 = draw(n)
            ref[bad], boxes[bad, 0:3], ref_theta[bad], boxes[bad, 6] = r2, x2, t2, (t2 + d2).astype(np.float32)
        else:
            raise AssertionError("the redraw did not converge")
    assert boxes.shape == (rows, 7) and ref.shape == (rows, 3)
    return dict(ref_pts=ref, ref_theta=ref_theta, boxes=boxes, mean_sizes=ms, cst=cst, redraws=redraws)


def exact_rows(t):
    """rows of a heading case whose rotated offsets are not finite: the clip sends them to a clamp, exact on both sides"""
    return ~(np.isfinite(t["rx"]) & np.isfinite(t["rz"]))


def accounting(c, t):
    """branch counts of an encode case, from the fp32 restatement"""
    cst = t["cst"]
    o, tr = encode(c["rcnn"], t["ref_pts"], t["ref_theta"], t["boxes"], t["mean_sizes"], cst)
    hi, two_s = cst["hi_xz"][None, :], (cst["ss"] + cst["ss"])[None, :]
    n = {}
    with np.errstate(invalid="ignore"):
        for a in ("x", "z"):
            tt, q = tr["t" + a], tr["q" + a]
            n[a + "_below"] = int((tt < 0).sum())
            n[a + "_above"] = int((tt > two_s).sum())
            n[a + "_at_lo"] = int((tt == 0).sum())
            n[a + "_at_hi"] = int((tt == two_s).sum())
            n[a + "_clamped_hi"] = int((tt > hi).sum())
            edge = (q == np.floor(q)) & (q > 0) & (tt < hi)
            n[a + "_edges"] = min(len(set(q[:, j][edge[:, j]].tolist())) for j in range(q.shape[1]))
            n[a + "_interior"] = int(((tt > 0) & (tt < hi)).sum())
        pre, lo_t, hi_t = tr["pre_t"], tr["lo_t"], tr["hi_t"]
        n.update(t_below=int((pre < lo_t).sum()), t_above=int((pre > hi_t).sum()), t_at_lo=int((pre == lo_t).sum()), t_inside=int(((pre > lo_t) & (pre < hi_t)).sum()))
        if not c["rcnn"]:
            n["t_at_2r"] = int((pre == cst["r"] + cst["r"]).sum())
        else:
            d0 = tr["d0"]
            n.update(first=int(((d0 > 0) & (d0 < tr["half_pi"])).sum()), fold=int(tr["fold"].sum()), last=int((d0 > tr["three_half"]).sum()),
                     at_half_pi=int((d0 == tr["half_pi"]).sum()), at_three_half=int((d0 == tr["three_half"]).sum()),
                     th0_negative=int((tr["th0"] < 0).sum()), th0_past_2pi=int((tr["th0"] > np.float32(2 * math.pi)).sum()))
    n["bins_in_range"] = bool(((o["bin_x"] >= 0) & (o["bin_x"] < cst["nbx"]) & (o["bin_z"] >= 0) & (o["bin_z"] < cst["nbx"])).all()
                              and ((o["bin_t"] >= 0) & (o["bin_t"] < cst["nbt"])).all())
    return n


# what each encode family is there for: keys of accounting() that must be positive (a tuple per rank where they differ)
_XZ_EDGES = tuple(a + s for a in ("x", "z") for s in ("_below", "_above", "_at_lo", "_at_hi", "_clamped_hi", "_interior"))
ENCODE_REACHES = {
    "dyadic": {0: _XZ_EDGES + ("t_below", "t_above", "t_at_lo", "t_at_2r", "t_inside"),
               1: _XZ_EDGES + ("t_below", "t_above", "t_inside", "first", "fold", "last", "at_half_pi", "at_three_half")},
    "background": {0: ("x_below", "x_above", "z_below")},
    "random": {0: ("x_below", "x_clamped_hi", "x_interior", "z_below", "z_clamped_hi", "t_below", "t_above", "t_inside"),
               1: ("x_below", "x_clamped_hi", "x_interior", "t_below", "t_above", "t_inside", "first", "fold", "last")},
    "nonfinite": {0: (), 1: ()},
}


def decode_inputs(c):
    cst = consts(c["params"])
    g = rng_of(c)
    rows, k, nbx, nbt = c["rows"], cst["k"], cst["nbx"], cst["nbt"]
    i = np.arange(rows)
    bins = {}
    for n, nb in (("bin_x", nbx), ("bin_z", nbx), ("bin_t", nbt)):
        b = g.integers(0, nb, (rows, k)).astype(np.int32)
        b[i % 5 == 0], b[i % 5 == 1] = 0, nb - 1
        bins[n] = b
    res = {}
    for j, n in enumerate(("res_x", "res_z", "res_t")):
        v = g.uniform(-0.5, 0.5, (rows, k)).astype(np.float32)
        for m, val in enumerate((0.5, -0.5, 0.75, -0.75)):
            v[(i + j) % 7 == m] = val
        res[n] = v
    ms = g.uniform(0.5, 4.0, (rows, k, 3)).astype(np.float32)
    ref = np.stack([g.uniform(-40, 40, rows), g.uniform(-2, 3, rows), g.uniform(0.5, 70, rows)], axis=1).astype(np.float32)
    th = {"none": None, "zero": np.zeros(rows, np.float32), "random": g.uniform(-7, 7, rows).astype(np.float32)}[c["heading"]]
    return dict(ref_pts=ref, ref_theta=th, res_y=g.uniform(-1, 1, (rows, k)).astype(np.float32), res_size=g.uniform(-0.3, 0.3, (rows, k, 3)).astype(np.float32),
                mean_sizes=ms, cst=cst, **bins, **res)


DECODE_ARGS = ("bin_x", "res_x", "bin_z", "res_z", "bin_t", "res_t", "res_y", "res_size", "mean_sizes")


def decode_ref(t, dt=np.float32, heading=True):
    return decode(t["ref_pts"], t["ref_theta"] if heading else None, *[t[n] for n in DECODE_ARGS], t["cst"], dt)


TIE = 10.0                                                  # far above the seeded N(0, 1) logits


def head_inputs(c):
    """finite logits; per slice and row pattern (row + slice) % 5: 0, 4 seeded; 1 the maximum tied in the first and the last position (the
    first wins); 2 tied in a middle and the last position (the middle wins); 3 strictly largest in the last position"""
    cst = consts(c["params"])
    g = rng_of(c)
    rows, k = c["rows"], c["k"]
    assert k == cst["k"]
    nbx, nbz, nbt = c["bins"]
    d = head_width(nbx, nbz, nbt)
    head = g.normal(0, 1, (rows, k, d)).astype(np.float32)
    i = np.arange(rows)
    want = {}
    for s, (start, nb) in enumerate(((0, nbx), (2 * nbx, nbz), (2 * nbx + 2 * nbz, nbt))):
        pat = (i + s) % 5
        last, mid = start + nb - 1, start + (nb - 1) // 2
        head[pat == 1, :, start], head[pat == 1, :, last] = TIE, TIE
        head[pat == 2, :, mid], head[pat == 2, :, last] = TIE, TIE
        head[pat == 3, :, last] = TIE
        want[s] = np.select([pat == 1, pat == 2, pat == 3], [0, (nb - 1) // 2, nb - 1], -1)
    ref = np.stack([g.uniform(-40, 40, rows), g.uniform(-2, 3, rows), g.uniform(0.5, 70, rows)], axis=1).astype(np.float32)
    th = {"none": None, "zero": np.zeros(rows, np.float32), "random": g.uniform(-7, 7, rows).astype(np.float32)}[c["heading"]]
    cls = None
    if c["cls"]:
        cls = g.integers(0, k, rows).astype(np.int32)
        cls[i % 11 == 3], cls[i % 11 == 7] = -1, k
    return dict(head=head, ref_pts=ref, ref_theta=th, mean_sizes_k=g.uniform(0.5, 4.0, (k, 3)).astype(np.float32), cls=cls, cst=cst, planted=want)


def head_ref(c, t, dt=np.float32, heading=True):
    return head_decode(t["head"], t["ref_pts"], t["ref_theta"] if heading else None, t["mean_sizes_k"], *c["bins"], t["cst"], dt=dt)


# exact projection family: the calibration is an axis permutation with a power-of-two focal length f: u = f y / x, v = f z / x, depth x
FOCAL = (2.0, 4.0)


def exact_calib(b):
    P = np.zeros((b, 3, 4), np.float32)
    for i in range(b):
        f = FOCAL[i % 2]
        P[i, 0, 1], P[i, 1, 2], P[i, 2, 0] = f, f, 1.0
    return P.reshape(b, 12)


def special_pixels(h, w):
    """(u, v, depth, what) with exact quotients"""
    big = float(2 ** 31)
    out = []
    for n, (us, fixed) in enumerate((((0, w - 1, w, -1, -0.5, -0.984375, w - 0.5, 1.5, big, -big, 2 * big, -2 * big, big - 128, -(big - 128)), 1.0),
                                     ((0, h - 1, h, -1, -0.5, -0.984375, h - 0.5, 1.5, big, -big, 2 * big, -2 * big, big - 128, -(big - 128)), 2.0))):
        for v in us:
            out.append(((v, fixed) if n == 0 else (fixed, v)) + (1.0, "edge"))
    return out


def gather_inputs(c):
    b, p, h, w, ch = c["b"], c["p"], c["h"], c["w"], c["c"]
    g = rng_of(c)
    img = g.normal(0, 1, (b, h, w, ch)).astype(np.float32)
    if c["family"] == "general":
        calib = np.array([[721.5377, 0.0, 609.5593, 44.85728, 0.0, 721.5377, 172.854, 0.2163791, 0.0, 0.0, 1.0, 0.002745884],
                          [707.0493, 0.0, 604.0814, 45.75831, 0.0, 707.0493, 180.5066, -0.3454157, 0.0, 0.0, 1.0, 0.004981016]], np.float32)[:b]
        # points whose pixel lies in and around a window of the image plane that the (h, w) map covers once the principal point is moved
        calib[:, 2], calib[:, 6] = w / 2.0, h / 2.0
        u, v, z = g.uniform(-4, w + 4, (b, p)), g.uniform(-3, h + 3, (b, p)), g.uniform(5, 60, (b, p))
        P = calib.astype(np.float64)[:, None, :]
        x = ((u * (z + P[..., 11])) - P[..., 3] - P[..., 2] * z) / P[..., 0]
        y = ((v * (z + P[..., 11])) - P[..., 7] - P[..., 6] * z) / P[..., 5]
        return dict(pts=np.stack([x, y, z], axis=-1).astype(np.float32), calib=calib, img=img)
    calib = exact_calib(b)
    pts = np.empty((b, p, 3), np.float32)
    for i in range(b):
        f = FOCAL[i % 2]
        if c["family"] == "tiles":          # every point inside the map, consecutive points on consecutive pixels: a shifted row shows
            j = np.arange(p) + 7 * i
            u, v, d = (j % w) + 0.5, ((j // w) % h) + 0.25, np.ones(p)
        else:
            u, v, d = g.integers(0, w, p) + 0.5, g.integers(0, h, p) + 0.25, 2.0 ** g.integers(-1, 3, p)
        pts[i] = np.stack([d, u * d / f, v * d / f], axis=1)
        if c["family"] == "exact":
            sp = special_pixels(h, w)
            for n, (uu, vv, dd, _) in enumerate(sp):
                pts[i, n] = (dd, uu * dd / f, vv * dd / f)
            n = len(sp)
            # depth 0 (+inf, NaN), -0.0 (-inf), negative depth with a pixel inside the map, NaN in each coordinate
            extra = [(0.0, 1.0, 1.0), (0.0, 0.0, 0.0), (-0.0, 1.0, 1.0), (-1.0, -2.0 / f, -1.0 / f), (np.nan, 1.0, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, np.nan),
                     (0.0, -1.0, 1.0)]
            for m, e in enumerate(extra):
                pts[i, n + m] = e
            assert n + len(extra) <= p
    return dict(pts=pts, calib=calib, img=img)


def gather_ref(c, t):
    pix, uf, vf = project(t["pts"], t["calib"])
    return gather(t["img"], pix), pix


def gather_grad_inputs(c):
    """integer-valued grad_out: every sum is an integer below 2^24, exact in any order; the last image row and pixel (0, 0) of frame 1
    receive nothing"""
    b, p, h, w, ch = c["b"], c["p"], c["h"], c["w"], c["c"]
    g = rng_of(c)
    pix = np.stack([g.integers(-2, w + 2, (b, p)), g.integers(-2, h - 1, (b, p))], axis=-1).astype(np.int32)
    if p:
        first = (pix[1, :, 0] == 0) & (pix[1, :, 1] == 0)
        pix[1, first, 0] = 1
    assert p * 2 < 2 ** 24
    return dict(pix=pix, grad_out=g.integers(-2, 3, (b, p, ch)).astype(np.float32))


def concat_inputs(c):
    g = rng_of(c)
    rows, c1, c2 = c["rows"], c["c1"], c["c2"]
    if c["op"] == "concat":
        return dict(a=g.normal(0, 1, (rows, c1)).astype(np.float32), b=g.normal(0, 1, (rows, c2)).astype(np.float32))
    return dict(grad_out=g.normal(0, 1, (rows, c1 + c2)).astype(np.float32))


# ------------------------------------------------------------------------------------------------- argument checks, no launch
def check_arguments():
    """every call returns before anything is launched (fake non-null pointers, never dereferenced); tests/test_glue_cases_cpu.py runs this
    without a GPU, tests/test_glue_abi.py on the GPU"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)
    E, OK = _lib.HF_EINVAL, _lib.HF_OK
    bad = {}

    def ptrs(n, null):
        return [None if i == null else fake for i in range(n)]

    def gather(b=1, p=4, h=3, w=5, c=4, null=None, pix=fake):
        return L.hf_project_gather(b, p, h, w, c, *ptrs(4, null), pix, None)           # pts calib img out

    def grad(b=1, p=4, h=3, w=5, c=4, null=None):
        return L.hf_project_gather_grad(b, p, h, w, c, *ptrs(3, null), None)           # grad_out pix grad_img

    def concat(rows=4, c1=4, c2=4, null=None):
        a, b, out = ptrs(3, null)
        return L.hf_fuse_concat(rows, c1, c2, a, b, None, out, None)

    def cgrad(rows=4, c1=4, c2=4, g=fake, ga=fake, gb=fake):
        return L.hf_fuse_concat_grad(rows, c1, c2, g, None, ga, gb, None)

    def decode(rows=4, k=3, null=None):
        p = ptrs(14, null)                  # ref_pts ref_theta(1) 9 per-class arrays ss deltas | boxes
        return L.hf_bin_box_decode(rows, k, *p[:13], 0.5, 0.25, p[13], None)

    def encode(rows=4, k=3, null=None):
        p = ptrs(15, null)                  # ref_pts ref_theta(1) boxes mean_sizes ss deltas hi_xz | 8 outputs
        return L.hf_bin_box_encode(rows, k, 0, *p[:7], 0.5, 0.999, 0.25, 0.125, *p[7:], None)

    def head(rows=4, k=3, nbx=2, nbz=2, nbt=2, null=None, cls=None):
        p = ptrs(7, null)                   # head ref_pts ref_theta(2) mean_sizes_k ss deltas | boxes
        return L.hf_bin_head_decode(rows, k, nbx, nbz, nbt, *p[:6], 0.5, 0.25, cls, p[6], None)

    for name, f in (("gather", gather), ("grad", grad)):
        bad.update({"%s: %s" % (name, k): f(**v) for k, v in (("b < 0", dict(b=-1)), ("p < 0", dict(p=-1)), ("h = 0", dict(h=0)), ("w = 0", dict(w=0)),
                                                               ("c = 0", dict(c=0)), ("h < 0", dict(h=-2)))})
    bad.update({"gather: pointer %d is NULL" % i: gather(null=i) for i in range(4)})
    bad.update({"grad: pointer %d is NULL" % i: grad(null=i) for i in range(3)})
    bad["grad: no grad_img for an empty point set"] = grad(p=0, null=2)
    for name, f in (("concat", concat), ("cgrad", cgrad)):
        bad.update({"%s: rows < 0" % name: f(rows=-1), "%s: c1 = 0" % name: f(c1=0), "%s: c2 = 0" % name: f(c2=0), "%s: c1 < 0" % name: f(c1=-4)})
    bad.update({"concat: pointer %d is NULL" % i: concat(null=i) for i in range(3)})
    bad["cgrad: no grad_out"] = cgrad(g=None)
    for name, f, n, optional in (("decode", decode, 14, (1,)), ("encode", encode, 15, (1,)), ("head", head, 7, (2,))):
        bad.update({"%s: rows < 0" % name: f(rows=-1), "%s: k = 0" % name: f(k=0), "%s: k < 0" % name: f(k=-1)})
        bad.update({"%s: pointer %d is NULL" % (name, i): f(null=i) for i in range(n) if i not in optional})
    bad.update({"head: nbx = 0": head(nbx=0), "head: nbz = 0": head(nbz=0), "head: nbt = 0": head(nbt=0), "head: nbx < 0": head(nbx=-3)})
    wrong = {k: v for k, v in bad.items() if v != E}
    assert not wrong, wrong
    # nothing to do: HF_OK with null pointers, nothing launched
    none = [None] * 15
    ok = {"gather: p = 0": L.hf_project_gather(2, 0, 3, 5, 4, None, None, None, None, None, None),
          "gather: b = 0": L.hf_project_gather(0, 7, 3, 5, 4, None, None, None, None, None, None),
          "grad: b = 0": L.hf_project_gather_grad(0, 7, 3, 5, 4, None, None, None, None),
          "concat: rows = 0": L.hf_fuse_concat(0, 4, 4, None, None, None, None, None),
          "cgrad: rows = 0": L.hf_fuse_concat_grad(0, 4, 4, None, None, None, None, None),
          "cgrad: both gradients NULL": cgrad(ga=None, gb=None), "cgrad: both NULL and no grad_out": cgrad(g=None, ga=None, gb=None),
          "decode: rows = 0": L.hf_bin_box_decode(0, 3, *none[:13], 0.5, 0.25, None, None),
          "encode: rows = 0": L.hf_bin_box_encode(0, 3, 1, *none[:7], 0.5, 0.999, 0.25, 0.125, *none[:8], None),
          "head: rows = 0": L.hf_bin_head_decode(0, 3, 2, 2, 2, *none[:6], 0.5, 0.25, None, None, None)}
    wrong = {k: v for k, v in ok.items() if v != OK}
    assert not wrong, wrong
