"""The case table, the restated launch rule, the references and the scatter bound of the row-gather family (csrc/row_gather.h):
group_point / group_point_into / gather_point / three_interpolate_cl and their gradients.  NumPy only: tests/test_row_gather_abi.py
runs the cases on the GPU through the C ABI, tests/test_row_gather_cases_cpu.py checks the table and the references themselves.

Expected values: the committed oracle (oracle.group_point*, three_interpolate*, gather_point*) where it has the form, and the
float32 NumPy restatement below where it has none (column slices); the CPU test asserts that the two agree on every case.
  forward          bit for bit (copy forms on arbitrary bit patterns, compared as int32)
  gather gradient  bit for bit: the restatement adds in ascending (row, slot) order, the order of the oracle's sequential loop
  scatter gradient within the bound of scatter_reference() of the fp64 sum of the exact products (the atomics add in no fixed order)"""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32
SENTINEL_BITS = 0x7fc5a5a5          # a NaN with a payload: untouched output floats must keep exactly these bits
NUM_CU = 256


def case_id(c):
    return c["name"]


# ---------------------------------------------------------------- forward
def _fwd(name, entry, c, regime, b=2, n=50, rows=(37, 3), width=None, col=0, off=None):
    """entry: group_point | group_point_into | gather_point | three_interpolate_cl; rows = (m, nsample) output rows per cloud;
    off: the operand handed over one float past a 16-byte boundary"""
    m, k = rows
    return dict(name=name, entry=entry, nsrc=3 if entry == "three_interpolate_cl" else 1, b=b, n=n, m=m, k=k, c=c,
                width=width or c, col=col, off=off, regime=regime)


def _both(name, c, regime, **kw):
    """the dense forward of both NSRC: group_point rows (m, k), three_interpolate_cl rows (m * k, 1)"""
    m, k = kw.pop("rows", (37, 3))
    return [_fwd("group_point/" + name, "group_point", c, regime, rows=(m, k), **kw),
            _fwd("three_interpolate_cl/" + name, "three_interpolate_cl", c, regime, rows=(m * k, 1), **kw)]


FORWARD_CASES = (
    _both("c16_pow2_lower", 16, "pow2") + _both("c1024_pow2_upper", 1024, "pow2") +
    _both("c2048_vec4", 2048, "vec4") + _both("c24_vec4", 24, "vec4") +
    _both("c5_scalar", 5, "scalar") + _both("c3_scalar", 3, "scalar") + _both("c1_scalar", 1, "scalar") +
    _both("c16_points_off", 16, "scalar", off="points") + _both("c16_out_off", 16, "scalar", off="out") +
    # more row pieces than one grid stride covers.  pow2: rows_per_batch * cv / 1024 > 2048 / b workgroups per cloud
    _both("c1024_pow2_many", 1024, "pow2", rows=(4099, 1)) +
    # generic: nrows * cv > 8 * 256 workgroups * 256 lanes; the dense c = 16 rows reach it through group_point_into only
    [_fwd("group_point_into/c16_vec4_many", "group_point_into", 16, "vec4", rows=(70001, 1)),
     _fwd("three_interpolate_cl/c24_vec4_many", "three_interpolate_cl", 24, "vec4", rows=(45001, 1)),
     _fwd("gather_point/50_37", "gather_point", 3, "scalar", rows=(37, 1)),
     _fwd("gather_point/1_1", "gather_point", 3, "scalar", b=1, n=1, rows=(1, 1)),
     _fwd("group_point_into/c16_w24_col8", "group_point_into", 16, "vec4", width=24, col=8),
     _fwd("group_point_into/c16_w19_col3", "group_point_into", 16, "scalar", width=19, col=3),
     _fwd("group_point_into/c7_w12_col5", "group_point_into", 7, "scalar", width=12, col=5),
     _fwd("group_point_into/c16_dense", "group_point_into", 16, "vec4")])    # dense rows, yet never the pow2 form


def forward_regime(c):
    """the launch rule of launch_gather_rows restated: which form a case reaches, and with how many workgroups"""
    rpb = c["m"] * c["k"]
    aligned = c["off"] is None
    vec4 = c["c"] % 4 == 0 and c["width"] % 4 == 0 and c["col"] % 4 == 0 and aligned
    cv = c["c"] // 4
    if (c["entry"] in ("group_point", "three_interpolate_cl") and vec4 and 4 <= cv <= 256 and cv & (cv - 1) == 0
            and c["b"] <= 65535 and rpb * cv < 2 ** 31):
        want = -(-rpb * cv // 1024)
        per_cloud = min(want, max(1, NUM_CU * 8 // c["b"]))
        return "pow2", per_cloud * c["b"], want > per_cloud
    items = c["b"] * rpb * (cv if vec4 else c["c"])
    want = -(-items // 256)
    return ("vec4" if vec4 else "scalar"), min(want, NUM_CU * 8), want > NUM_CU * 8


def forward_inputs(c):
    """points (b, n, c), idx (b, rows, nsrc) int32, weight (b, rows, 3) or None.  Copy forms carry arbitrary bit patterns
    (NaN payloads, -0.0, denormals, infinities): they must move bits."""
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    rows = c["m"] * c["k"]
    idx = rng.integers(0, c["n"], (c["b"], rows, c["nsrc"])).astype(np.int32)
    if c["nsrc"] == 1:
        points = rng.integers(0, 2 ** 32, (c["b"], c["n"], c["c"]), dtype=np.uint64).astype(np.uint32).view(np.float32)
        points.reshape(-1)[:2] = np.array([0x80000000, 0x7fa00001], np.uint32).view(np.float32)   # -0.0, a signalling NaN
        return points, idx, None
    points = rng.standard_normal((c["b"], c["n"], c["c"])).astype(np.float32)
    weight = rng.random((c["b"], rows, 3), dtype=np.float32)
    return points, idx, weight


def forward_restated(points, idx, weight):
    """float32 NumPy: the copy moves bits; the weighted sum is w0*p0 + w1*p1 + w2*p2 left to right, every product and sum
    rounded to float32 (no fused multiply-add).  -> (b, rows, c)"""
    bidx = np.arange(points.shape[0])[:, None]
    if weight is None:
        return points[bidx, idx[:, :, 0]]
    p = [points[bidx, idx[:, :, t]] for t in range(3)]
    w = [weight[:, :, t, None] for t in range(3)]
    return (w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]


def forward_oracle(oracle, c, points, idx, weight):
    b, rows = idx.shape[:2]
    if c["entry"] == "gather_point":
        return oracle.gather_point(points, idx[:, :, 0])
    if c["nsrc"] == 1:
        return oracle.group_point(points, idx.reshape(b, c["m"], c["k"])).reshape(b, rows, c["c"])
    return oracle.three_interpolate(points, idx, weight)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---------------------------------------------------------------- gradient in gather form
def _gg(name, nsrc, c, vec4, ld=None, col=0, b=2, n=41, rows=111, off=False):
    """n target rows per cloud, `rows` rows of grad_out per cloud (stride ld, columns from col).  The weighted entry with a row
    stride (hf_three_interpolate_concat_grad) has no column argument -- its columns come first -- so ld > c goes with col > 0 for
    the copy and with col = 0 for the weighted form"""
    return dict(name="%s/%s" % ("group_point_grad_gather" if nsrc == 1 else "three_interpolate_grad_gather", name), nsrc=nsrc,
                b=b, n=n, rows=rows, c=c, ld=ld or c, col=col, off=off, vec4=vec4)


GATHER_GRAD_CASES = (
    [_gg("c16_vec4", s, 16, True) for s in (1, 3)] + [_gg("c5_scalar", s, 5, False) for s in (1, 3)] +
    [_gg("c16_off_scalar", s, 16, False, off=True) for s in (1, 3)] +
    [_gg("c300_scalar_block320", s, 300, False, off=True) for s in (1, 3)] +          # cv > 256: the block is rounded up to 320
    [_gg("c1028_vec4_block320", s, 1028, True) for s in (1, 3)] +                     # cv = 257
    [_gg("c16_ld24_col8_vec4", 1, 16, True, ld=24, col=8), _gg("c16_ld19_col3_scalar", 1, 16, False, ld=19, col=3),
     _gg("c7_ld12_col5_scalar", 1, 7, False, ld=12, col=5),
     _gg("c16_ld24_vec4", 3, 16, True, ld=24), _gg("c16_ld19_scalar", 3, 16, False, ld=19), _gg("c7_ld12_scalar", 3, 7, False, ld=12)])


def gather_grad_block(c):
    """launch_grad_gather_rows restated: (16-byte form?, lanes per target row, workgroup size)"""
    vec4 = c["c"] % 4 == 0 and c["ld"] % 4 == 0 and c["col"] % 4 == 0 and not c["off"]
    cv = c["c"] // 4 if vec4 else c["c"]
    return vec4, cv, 256 if cv <= 256 else (cv + 63) // 64 * 64


def grad_inputs(c):
    """idx (b, rows, nsrc) with a hub named by every row and a target that nothing names, weight, grad_out (b, rows, ld) whose
    columns outside [col, col + c) are NaN: they must not be read"""
    rng = np.random.default_rng(sum(map(ord, c["name"])))
    n = c["n"]
    idx = rng.integers(0, n, (c["b"], c["rows"], c["nsrc"])).astype(np.int32)
    if n > 2:
        idx[idx == n - 1] = 0          # target n-1: no entries
        idx[:, :, 0] = 7 % n           # a hub
    weight = rng.random((c["b"], c["rows"], 3), dtype=np.float32) if c["nsrc"] == 3 else None
    wide = np.full((c["b"], c["rows"], c["ld"]), np.nan, np.float32)
    wide[:, :, c["col"]:c["col"] + c["c"]] = rng.standard_normal((c["b"], c["rows"], c["c"])).astype(np.float32)
    return idx, weight, wide


def addends(c, idx, weight, wide, dtype):
    """target row (b, rows * nsrc) and addend (b, rows * nsrc, c) of every (row, slot), in `dtype`: float32 rounds the
    product go * w as the kernels do, float64 holds it exactly (24 x 24 bits)"""
    go = wide[:, :, c["col"]:c["col"] + c["c"]].astype(dtype)
    if c["nsrc"] == 1:
        return idx[:, :, 0], go
    return idx.reshape(idx.shape[0], -1), (go[:, :, None, :] * weight.astype(dtype)[:, :, :, None]).reshape(idx.shape[0], -1, c["c"])


def grad_sequential(c, idx, weight, wide):
    """float32, one addend after the other in ascending (row, slot) order: np.add.at is unbuffered and walks its index
    in order -- the restatement of the reference's sequential loop, which the gather form must equal bit for bit"""
    tgt, add = addends(c, idx, weight, wide, np.float32)
    g = np.zeros((c["b"], c["n"], c["c"]), np.float32)
    np.add.at(g, (np.arange(c["b"])[:, None], tgt), add)
    return g


def grad_oracle(oracle, c, idx, weight, wide):
    go = np.ascontiguousarray(wide[:, :, c["col"]:c["col"] + c["c"]])
    shape = (c["b"], c["n"], c["c"])
    if c["nsrc"] == 1:
        return oracle.group_point_grad(shape, idx.reshape(c["b"], c["rows"], 1), go[:, :, None, :])
    return oracle.three_interpolate_grad(shape, idx, weight, go)


# ---------------------------------------------------------------- gradient in scatter form
def _sc(entry, c, nsrc=1, ld=None, col=0, b=2, n=41, rows=111):
    return dict(name="%s/c%d" % (entry, c), entry=entry, nsrc=nsrc, b=b, n=n, rows=rows, c=c, ld=ld or c, col=col, off=False)


SCATTER_CASES = [
    _sc("gather_point_grad", 3), _sc("group_point_grad", 16), _sc("group_point_grad", 5),
    _sc("group_point_grad_from", 16, ld=24, col=8), _sc("group_point_grad_from", 7, ld=12, col=5),
    _sc("group_concat_grad", 13, ld=16, col=3), _sc("group_concat_grad", 5, ld=8, col=0),     # xyz first / xyz last
    _sc("three_interpolate_cl_grad", 16, nsrc=3), _sc("three_interpolate_cl_grad", 5, nsrc=3)]


def scatter_reference(c, idx, weight, wide):
    """-> (fp64 sum of the exact addends, bound) per target element.
    Bound, derived: a target element receives t addends a_1 .. a_t.  Each float32 addend carries at most one rounding (the
    product go * w; none for a copy): |fl(a_i) - a_i| <= u |a_i|.  Adding t numbers into a zero in ANY order takes t - 1
    roundings beyond the first exact 0 + a, each of at most u |partial sum| <= u sum|a_i| (1 + O(t u)).  Together
    <= u sum|a| + (t - 1) u sum|a| = t u sum|a| to first order; (t + 1) u sum|a| covers the second-order terms for every
    t u << 1 (t <= a few hundred here).  An element that nothing names has t = 0 and sum|a| = 0: exactly zero."""
    tgt, add = addends(c, idx, weight, wide, np.float64)
    bidx = np.arange(c["b"])[:, None]
    shape = (c["b"], c["n"], c["c"])
    ref, mag, cnt = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    np.add.at(ref, (bidx, tgt), add)
    np.add.at(mag, (bidx, tgt), np.abs(add))
    np.add.at(cnt, (bidx, tgt), 1.0)
    return ref, (cnt + 1) * U * mag


def scatter_shuffled(c, idx, weight, wide, seed):
    """float32 summation of the same addends in a shuffled order: what an arbitrary order of the atomics may produce"""
    tgt, add = addends(c, idx, weight, wide, np.float32)
    g = np.zeros((c["b"], c["n"], c["c"]), np.float32)
    rng = np.random.default_rng(seed)
    for bb in range(c["b"]):
        order = rng.permutation(tgt.shape[1])
        np.add.at(g[bb], tgt[bb][order], add[bb][order])
    return g
