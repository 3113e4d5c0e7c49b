"""The case table and the NumPy restatement of the two sampler files, csrc/rpn_batch.hip (view filter, point sampling, labels, image)
and csrc/rcnn_targets.hip (3D IoU, RoI sampling, RoI jitter).  Imports neither the library nor torch.

Both files draw their random numbers from a counter hash (splitmix64 of a key and a counter), pure integer arithmetic, and the library
is built with -ffp-contract=off.  So this module predicts every index draw for draw, and every fp32 / fp64 output made of + - * / bit
for bit: tests/test_sampler_abi.py compares the kernels with it by np.array_equal; tests/test_sampler_cases_cpu.py checks this module
itself (bijection, statistics of the streams, branch accounting, the conditions below) without a GPU.

Everything here is restated from the kernels' text, nothing is imported from the package: the mixer, the keys, the keyed permutation
(4 Feistel rounds on the next even power of two, cycle-walked), rb_index, tgt_uniform / tgt_index, the draw numbers, the Box-Muller
forms, the placement branches, the target branches and the jitter loop.

Conditions on the inputs (asserted by the generators, they are no tolerance on the kernel), DELTA = 1e-4, about ten times the agreement
tests/test_rcnn_train.py demands of the device IoU against fp64:
  * no per-RoI maximum lies within DELTA of fg_thresh, neg_lo or neg_hi; the best and the second-best IoU of every RoI row and GT column
    differ by more than DELTA unless the two boxes are bit-identical (or both are exactly 0: see below); every pair has fp64 IoU 0 or
    >= DELTA; a pair with IoU 0 has no height overlap or a separating-axis gap of at least 1 cm in BEV, so the device's fp32 overlap is
    exactly 0 as well and a tie at 0 resolves to the first index on both sides;
  * no try of the jitter loop of any slot has an fp64 IoU within DELTA of fg_thresh: the generator walks seeds 0, 1, 2, ... (the RNG seed
    where the case leaves the state free, the data seed where it fixes the state) and keeps the first that holds;
  * view filter: |u|, |u - W|, |v|, |v - H|, |z|, |z - 40| are exactly 0 (the boundary points, exact by construction: the calibration is
    an axis permutation and a power-of-two focal length) or >= 1e-6.

A property of the keyed permutation, recorded and not changed here: with 4 Feistel rounds whose round function is masked to half the
(even) bit count, the permutation is measurably non-uniform on tiny domains.  A host prototype gives, over 20 000 keys, single-element
inclusion counts 11 sigma off at n = 5 and a position chi-square of 580 against 361 degrees of freedom at n = 20; from n = 64 up it
is indistinguishable from uniform (4034 against 3969 at n = 64, 89 858 against 89 401 at n = 300).  The training path permutes domains
of thousands of points.  Changing the hash would change every seeded run and the exported hand-off files, so below 64 the tests assert
bijection only.
"""
import functools
import math

import numpy as np

import kitti_data_np as KN

U = 2.0 ** -24
DELTA = 1e-4
GAP = 0.01
VIEW_MARGIN = 1e-6
ELU_FACTOR = 4                     # the house rule of gemm_cases.py: bound = 4 x the error of the fp32 CPU form against fp64
M64 = (1 << 64) - 1
_C1, _C2, _C3 = np.uint64(0x9e3779b97f4a7c15), np.uint64(0xbf58476d1ce4e5b9), np.uint64(0x94d049bb133111eb)
_CALL = 0xd1b54a32d192ed03
NEAR, FAR, EXTRA, DRAW, SHUFFLE, NORMAL = 1, 2, 3, 4, 5, 6          # purposes of rb_key
DRAW_PERM, DRAW_INDEX, DRAW_JITTER = 0, 1, 16                      # draw numbers of tgt_uniform
FG_TRIES, BG_TRIES = 10, 1
STATUS_EMPTY, STATUS_TOO_MANY_FAR = 1, 2
AUG_METHODS = {"": 0, "none": 0, "single": 1, "multiple": 2, "normal": 3}
THREADS = 256
FAR_DEPTH = 40.0
TGT_MAX_R = 512
IMG_PIX_PER_BLOCK, IMG_MAX_SIDE, IMG_MAX_PIXELS = 256 * 16, 8192, 1 << 23
SENT_I = -7


# ================================================================================================ the counter hash
def u64(x):
    return np.uint64(int(x) & M64)


def mix(z):
    """rb_mix == splitmix64, on uint64 arrays (wrap-around arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _C1
        z = (z ^ (z >> np.uint64(30))) * _C2
        z = (z ^ (z >> np.uint64(27))) * _C3
    return z ^ (z >> np.uint64(31))


def tgt_key(seed, call):
    """the key of one call: [seed, call] read as uint64"""
    return mix(u64((int(seed) & M64) + (int(call) & M64) * _CALL))


def rb_key(seed, call, frame, purpose):
    return mix(tgt_key(seed, call) ^ u64((int(frame) << 8) | int(purpose)))


def perm_bits(n):
    bits = 2
    while (1 << bits) < n:
        bits += 1
    return bits + (bits & 1)


def rb_apply(key, n, x):
    """the keyed bijection of [0, n) applied to x (array); key a scalar or an array of x's shape"""
    half = perm_bits(n) // 2
    h, mask = np.uint64(half), np.uint64((1 << half) - 1)
    x = np.asarray(x, dtype=np.uint64)
    shape = x.shape
    keys = np.broadcast_to(np.asarray(key, dtype=np.uint64), shape).reshape(-1)
    out = x.reshape(-1).copy()
    todo = np.arange(out.size)
    while todo.size:                                    # do ... while (x >= n)
        v, k = out[todo], keys[todo]
        l, r = v >> h, v & mask
        for rnd in range(4):
            f = mix(k ^ (np.uint64(rnd << 32) | r)) & mask
            l, r = r, l ^ f
        v = (l << h) | r
        out[todo] = v
        todo = todo[v >= np.uint64(n)]
    return out.reshape(shape).astype(np.int64)


def rb_index(key, i, n):
    """uniform index in [0, n) of draw i under key"""
    hi = mix(np.asarray(key, np.uint64) ^ mix(np.asarray(i, np.uint64))) >> np.uint64(32)
    return ((hi * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def tgt_uniform(key, frame, slot, draw):
    """float32 in [0, 1), 24 bits; counter frame << 40 | slot << 16 | draw"""
    ctr = (np.uint64(int(frame) << 40) | (np.asarray(slot, np.uint64) << np.uint64(16))) | np.asarray(draw, np.uint64)
    bits = mix(np.asarray(key, np.uint64) ^ mix(ctr)) >> np.uint64(40)
    return bits.astype(np.float32) * np.float32(1.0 / 16777216.0)


def tgt_index(u, size):
    """floor of the float32 product, capped at size - 1"""
    i = np.floor(np.asarray(u, np.float32) * np.float32(size)).astype(np.int64)
    return np.minimum(i, size - 1)


def image_normals(key):
    """the three N(0, 1) of a frame's noise vector: Box-Muller in fp64, u1 in (0, 1] from >> 11"""
    j = np.arange(3, dtype=np.uint64)
    a = (mix(key ^ mix(np.uint64(2) * j)) >> np.uint64(11)).astype(np.float64)
    b = (mix(key ^ mix(np.uint64(2) * j + np.uint64(1))) >> np.uint64(11)).astype(np.float64)
    u1, u2 = (a + 1.0) * (1.0 / 9007199254740992.0), b * (1.0 / 9007199254740992.0)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def state_after(state, calls=1):
    """[seed, call] as int64 after `calls` calls"""
    call = (int(state[1]) + calls) & M64
    return np.array([int(state[0]), call - (1 << 64) if call >= (1 << 63) else call], dtype=np.int64)


def align256(v):
    return (v + 255) & ~255


def rpn_points_workspace(b, total, max_frame):
    chunks = -(-max_frame // THREADS) if max_frame > 0 else 1
    return 256 + align256(total) + align256(8 * b * chunks) + align256(16 * b) + align256(4 * total)


def rpn_image_workspace(b, max_pixels):
    chunks = -(-max_pixels // IMG_PIX_PER_BLOCK) if max_pixels > 0 else 1
    return 256 + align256(72 * b * chunks)


def rcnn_targets_workspace(b, m, g):
    return align256(4 * b * m * g) + align256(4 * b * TGT_MAX_R) + 256


# ================================================================================================ the case table
W_IMG, H_IMG, FOCAL, CX, CY = 64, 32, 64.0, 32.0, 16.0
VELO_TO_RECT = np.array([[0, -1, 0, 0], [0, 0, -1, 0], [1, 0, 0, 0]], np.float64)          # x = -vy, y = -vz, z = vx
P2 = np.array([[FOCAL, 0, CX, 0], [0, FOCAL, CY, 0], [0, 0, 1, 0]], np.float64)


def _pts(p, frames, state=(7, 0), calls=1, clamp=False):
    """frames: (raw points, near in view, far in view, flip)"""
    return dict(kind="points", p=p, frames=tuple(frames), state=tuple(state), calls=calls, clamp=clamp)


def _points_cases():
    big = (-1, 2 ** 40 + 3)
    return [
        _pts(1, [(1, 1, 0, 0), (0, 0, 0, 0), (63, 0, 5, 1), (64, 3, 0, 0), (65, 1, 0, 1)]),
        _pts(2, [(1, 1, 0, 1), (255, 0, 2, 0), (256, 1, 2, 0), (257, 5, 1, 1)], state=big),
        _pts(3, [(1, 1, 0, 0), (64, 2, 0, 1), (65, 4, 4, 0), (0, 0, 0, 0), (63, 10, 1, 0)], calls=2),
        _pts(4, [(256, 2, 0, 0), (257, 1, 1, 1), (513, 100, 4, 0), (1000, 0, 300, 1)], clamp=True),
        _pts(5, [(1, 1, 0, 1), (64, 2, 0, 0), (255, 200, 3, 1), (256, 0, 5, 0), (257, 3, 1, 0)], state=big, calls=2),
        _pts(16, [(513, 300, 100, 0), (1000, 500, 16, 1), (1000, 400, 0, 0), (1000, 300, 10, 1), (1, 1, 0, 0)]),
        _pts(17, [(64, 8, 0, 1), (65, 4, 4, 0), (255, 10, 7, 0), (256, 9, 0, 1), (257, 0, 1, 0)], clamp=True),
        _pts(64, [(1000, 40, 24, 0), (513, 20, 20, 1), (257, 16, 16, 0), (256, 3, 3, 1), (0, 0, 0, 0)], state=big),
        _pts(100, [(1000, 600, 150, 1), (1000, 600, 100, 0), (513, 50, 0, 0), (255, 60, 30, 1), (63, 30, 19, 0)]),
        _pts(256, [(1000, 500, 100, 0), (513, 256, 0, 1), (257, 128, 0, 0), (257, 100, 27, 1), (64, 10, 10, 0)], calls=2),
        _pts(257, [(1000, 600, 200, 1), (1000, 0, 258, 0), (513, 128, 0, 0), (256, 200, 56, 1), (1, 1, 0, 0)]),
        _pts(1000, [(1000, 900, 100, 0), (1000, 400, 100, 1), (1000, 600, 300, 0), (513, 99, 1, 1), (257, 200, 49, 0)], state=big),
    ]


def _lab(b, p, g, layout, counts, expand):
    return dict(kind="labels", b=b, p=p, g=g, layout=tuple(layout), counts=tuple(counts), expand=expand)


def _labels_cases():
    out = []
    for cnt in (0, -3):
        out.append(_lab(1, 1, 0, ["none"], [cnt], 0.2))
    for cnt in (1, 6, 0, -3):
        for e in (0.0, 0.2):
            out.append(_lab(1, 5, 1, ["aligned"], [cnt], e))
    for cnts in ((3, 3), (3, 8), (0, 3), (-3, 2)):
        for e in (0.0, 0.2):
            out.append(_lab(2, 257, 3, ["nested", "rotated"], cnts, e))
    for cnt in (128, 133, 0):
        out.append(_lab(1, 300, 128, ["rotated"], [cnt], 0.2))
    out.append(_lab(1, 300, 128, ["rotated"], [128], 0.0))
    return out


def _img(src, out, frames, state=(7, 0), calls=1):
    """src (w, h), out (w, h); frames: (flip, jitter, special) with special in
    None / 'w0' / 'h8193' / 'past' / 'pixel' (a single-pixel source) / 'const'"""
    return dict(kind="image", src=tuple(src), out=tuple(out), frames=tuple(frames), state=tuple(state), calls=calls)


def _image_cases():
    four = [(0, 0, None), (1, 0, None), (0, 1, None), (1, 1, None)]
    big = (-1, 2 ** 40 + 3)
    return [
        _img((1, 1), (3, 2), four),
        _img((5, 7), (5, 7), four, state=big),
        _img((8, 6), (16, 12), four, calls=2),
        _img((6, 8), (3, 16), four),
        _img((64, 64), (7, 3), four, state=big, calls=2),
        _img((4097, 1), (33, 1), four),
        _img((5, 4), (4, 3), [(0, 1, "w0"), (1, 0, "h8193"), (0, 1, "past"), (1, 1, "pixel"), (0, 1, "const")]),
    ]


def _fr(n, ng, fg=0, hard=0, easy=None, pc=None, gc=None, far_gt=False, twin_gt=False, twin_roi=False, high=0):
    """one frame of a target case: n valid proposals (fg near a GT, hard shifted off a GT, high = above a GT with no height overlap,
    the rest easy = IoU 0), ng valid GTs; pc / gc the count the call is given (None: n / ng); far_gt: no proposal touches a GT"""
    easy = n - fg - hard - high if easy is None else easy
    assert fg + hard + high + easy == n and easy >= 0
    return dict(n=n, ng=ng, fg=fg, hard=hard, high=high, easy=easy, pc=n if pc is None else pc, gc=ng if gc is None else gc,
                far_gt=far_gt, twin_gt=twin_gt, twin_roi=twin_roi)


def _tgt(b, m, g, r, frames, aug=0, train=1, state=None, calls=1, fg_ratio=0.5, hard_ratio=0.8, neg=(0.05, 0.45)):
    """state None: [walked seed, 0]"""
    assert len(frames) == b and (train or r == m)
    return dict(kind="targets", b=b, m=m, g=g, r=r, frames=tuple(tuple(sorted(f.items())) for f in frames), aug=aug, train=train,
                state=None if state is None else tuple(state), calls=calls, fg_ratio=fg_ratio, hard_ratio=hard_ratio, neg=tuple(neg),
                pos=(0.6, 0.55))


def _targets_cases():
    big = (-1, 2 ** 40 + 3)
    out = []
    # (1, 1, 1, 1): one proposal on its GT -> fg only
    out.append(_tgt(1, 1, 1, 1, [_fr(1, 1, fg=1)], aug="multiple", state=(7, 0)))
    out.append(_tgt(1, 1, 1, 1, [_fr(1, 1, easy=1, far_gt=True)], aug=1))                     # bg only, easy only
    out.append(_tgt(1, 1, 1, 1, [_fr(1, 1, fg=1)], train=0))
    # (2, 5, 0, 4): no GT at all (the gt pointer is null): bg only, jitter on and no try
    out.append(_tgt(2, 5, 0, 4, [_fr(5, 0), _fr(3, 0)], aug=2, state=big))
    out.append(_tgt(2, 5, 0, 4, [_fr(5, 0, pc=8), _fr(0, 0, pc=-2)], aug=3))
    out.append(_tgt(2, 5, 0, 5, [_fr(5, 0), _fr(0, 0)], train=0))
    # (3, 64, 3, 7): fg_per_image at the ties (3.5 -> 4, 2.5 -> 2, 1.5 -> 2), nfg below / above it, nfg == 1
    f3 = [_fr(40, 3, fg=1, hard=1, high=2), _fr(64, 3, fg=20, hard=10, gc=5, twin_roi=True), _fr(30, 1, hard=1)]
    out.append(_tgt(3, 64, 3, 7, f3, aug="single"))
    out.append(_tgt(3, 64, 3, 5, f3, aug=2, state=(7, 0), calls=2))
    out.append(_tgt(3, 64, 3, 3, f3, aug="normal", hard_ratio=1.0))
    out.append(_tgt(3, 64, 3, 7, f3, aug=0, fg_ratio=0.0, hard_ratio=0.0))
    out.append(_tgt(3, 64, 3, 7, f3, aug=1, fg_ratio=1.0, state=big))
    out.append(_tgt(3, 64, 3, 64, f3, train=0))
    # (2, 257, 5, 64): the second trip of the per-RoI loop
    f4 = [_fr(257, 5, fg=60, hard=50, high=7, twin_gt=True), _fr(200, 4, fg=3, hard=100, easy=0, high=97, pc=200)]
    out.append(_tgt(2, 257, 5, 64, f4, aug="normal"))
    out.append(_tgt(2, 257, 5, 64, f4, aug="single", hard_ratio=0.0, state=big, calls=2))
    out.append(_tgt(2, 257, 5, 257, f4, train=0))
    # (1, 512, 128, 512): the limits; the second trip of the per-slot loop
    f5 = [_fr(512, 128, fg=200, hard=150, high=12, pc=515, gc=130)]
    out.append(_tgt(1, 512, 128, 512, f5, aug="multiple"))
    out.append(_tgt(1, 512, 128, 512, f5, train=0))
    # (4, 40, 4, 5): the counts outside their ranges, hard only / easy only, twins
    f6 = [_fr(0, 4, pc=-2), _fr(40, 4, fg=6, hard=12, pc=43, gc=6, twin_gt=True, twin_roi=True),
          _fr(25, 0, gc=-1), _fr(33, 2, fg=0, hard=33, easy=0, gc=2)]
    out.append(_tgt(4, 40, 4, 5, f6, aug=2))
    out.append(_tgt(4, 40, 4, 5, f6, aug=3, state=(7, 0), calls=2))
    out.append(_tgt(4, 40, 4, 40, f6, train=0))
    f7 = [_fr(0, 4, pc=0), _fr(12, 3, easy=12, far_gt=True), _fr(20, 2, fg=5, hard=0), _fr(9, 0, gc=0)]
    out.append(_tgt(4, 40, 4, 5, f7, aug=2, hard_ratio=1.0))
    # neither fg nor bg: with cls_neg_iou_range (0, 0) an IoU of 0 is neither easy (< 0) nor hard
    out.append(_tgt(4, 40, 4, 5, f7, aug="multiple", neg=(0.0, 0.0)))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(_points_cases() + _labels_cases() + _image_cases() + _targets_cases())


def cases_of(kind):
    return [c for c in all_cases() if c["kind"] == kind]


def _st(c):
    s = c["state"]
    return "walk" if s is None else ("s%dc%d" % s).replace("-", "m")


def case_id(c):
    k = c["kind"]
    if k == "points":
        return "points-p%d-%s-%s-x%d%s" % (c["p"], "_".join("%d.%d.%d%s" % (f[0], f[1], f[2], "f" if f[3] else "") for f in c["frames"]),
                                           _st(c), c["calls"], "-clamp" if c["clamp"] else "")
    if k == "labels":
        return "labels-b%d-p%d-g%d-%s-n%s-e%g" % (c["b"], c["p"], c["g"], "_".join(c["layout"]),
                                                   "_".join(str(n).replace("-", "m") for n in c["counts"]), c["expand"])
    if k == "image":
        return "image-%dx%d-to-%dx%d-%s-%s-x%d" % (c["src"] + c["out"] + ("_".join("%d%d%s" % (f[0], f[1], f[2] or "") for f in c["frames"]),
                                                                            _st(c), c["calls"]))
    fr = "_".join(("%d.%d.%d.%d" % (dict(f)["pc"], dict(f)["gc"], dict(f)["fg"], dict(f)["hard"])).replace("-", "m") for f in c["frames"])
    return "targets-b%d-m%d-g%d-r%d-%s-aug%s-%s-%s-x%d-fr%g-hr%g-neg%g" % (
        c["b"], c["m"], c["g"], c["r"], fr, c["aug"], "train" if c["train"] else "val", _st(c), c["calls"], c["fg_ratio"],
        c["hard_ratio"], c["neg"][1])


# ================================================================================================ RPN points
def classify(points, m, p2, wh):
    """0 out of view, 1 near, 2 far per raw row: the fp64 transform in the kernel's written order -> (cls, rect (N, 3), margins)"""
    px, py, pz = (points[:, d].astype(np.float64) for d in range(3))
    x = m[0] * px + m[1] * py + m[2] * pz + m[3]
    y = m[4] * px + m[5] * py + m[6] * pz + m[7]
    z = m[8] * px + m[9] * py + m[10] * pz + m[11]
    u = p2[0] * x + p2[1] * y + p2[2] * z + p2[3]
    v = p2[4] * x + p2[5] * y + p2[6] * z + p2[7]
    w = p2[8] * x + p2[9] * y + p2[10] * z + p2[11]
    with np.errstate(divide="ignore", invalid="ignore"):
        pu, pv = u / w, v / w
        inside = (z > 0.0) & (pu > 0.0) & (pu < float(wh[0])) & (pv > 0.0) & (pv < float(wh[1]))
    cls = np.where(inside, np.where(z < FAR_DEPTH, 1, 2), 0).astype(np.int64)
    front = z > 0.0
    with np.errstate(invalid="ignore"):
        px_margin = np.min(np.abs(np.stack([pu, pu - wh[0], pv, pv - wh[1]], 1)), axis=1)
    margin = np.minimum(np.where(front, px_margin, np.inf), np.minimum(np.abs(z), np.abs(z - FAR_DEPTH)))
    return cls, np.stack([x, y, z], 1), margin


def _frame_points(rng, raw, nn, nf):
    """raw rows of which exactly nn are near and nf far in view; the rest behind the camera, outside the image, or exactly on a bound
    (z == 0, u == 0, u == W, v == 0, v == H: strictly excluded); one far point sits at z == 40.0 exactly (far, not near)"""
    assert nn + nf <= raw
    rows = []

    def in_view(k, zlo, zhi):
        z = rng.uniform(zlo, zhi, k).astype(np.float32)
        x = (z * rng.uniform(-0.45, 0.45, k)).astype(np.float32)
        y = (z * rng.uniform(-0.2, 0.2, k)).astype(np.float32)
        return np.stack([x, y, z], 1)
    near, far = in_view(nn, 1.0, 39.0), in_view(nf, 41.0, 70.0)
    if nf:
        far[0] = (1.0, -2.0, 40.0)
    rows += [near, far]
    k = raw - nn - nf
    special = np.array([(1.0, 1.0, 0.0), (-4.0, 1.0, 8.0), (4.0, 1.0, 8.0), (1.0, -2.0, 8.0), (1.0, 2.0, 8.0), (0.5, 0.25, -3.0)], np.float32)[:k]
    rest = in_view(k - len(special), 1.0, 70.0)
    side = rng.integers(0, 3, len(rest))
    rest[side == 0, 2] *= -1                                        # behind the camera
    rest[side == 1, 0] = rest[side == 1, 2] * np.float32(0.75)      # u = 80 > W
    rest[side == 2, 1] = rest[side == 2, 2] * np.float32(-0.5)      # v = -16 < 0
    rect = np.concatenate(rows + [special, rest], 0).astype(np.float32)
    rect = rect[rng.permutation(raw)]
    pts = np.stack([rect[:, 2], -rect[:, 0], -rect[:, 1], rng.uniform(0, 1, raw).astype(np.float32)], 1).astype(np.float32)
    return pts


def _points_inputs(c):
    rng = np.random.default_rng(1000 + c["p"])
    frames = c["frames"]
    b = len(frames)
    parts = [_frame_points(rng, raw, nn, nf) for raw, nn, nf, _ in frames]
    points = np.concatenate(parts, 0) if parts else np.zeros((0, 4), np.float32)
    total = len(points)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    if c["clamp"]:
        offsets[0], offsets[-1] = -3, total + 9
    t = dict(points=points, offsets=offsets, velo_to_rect=np.tile(VELO_TO_RECT.reshape(1, 12), (b, 1)), p2=np.tile(P2.reshape(1, 12), (b, 1)),
             wh=np.tile(np.array([[W_IMG, H_IMG]], np.int32), (b, 1)), flip=np.array([f[3] for f in frames], np.int32),
             state=np.array(c["state"], np.int64), total=total, max_frame=max(f[0] for f in frames))
    for f, (raw, nn, nf, _) in enumerate(frames):
        cls, _, margin = classify(parts[f], t["velo_to_rect"][f], t["p2"][f], t["wh"][f])
        assert (cls == 1).sum() == nn and (cls == 2).sum() == nf, (f, (cls == 1).sum(), (cls == 2).sum())
        assert ((margin == 0) | (margin >= VIEW_MARGIN)).all(), "a point within %g of a view bound" % VIEW_MARGIN
    return t


def placement_branch(p, nn, nf):
    n = nn + nf
    if n == 0:
        return "empty"
    if p < n:
        if nf > p:
            return "far_only"
        if nf == p:
            return "near_none"
        return "far_none" if nf == 0 else "mixed"
    if p == n:
        return "equal"
    if p < 2 * n:
        return "extra_perm"
    if p == 2 * n:
        return "double"
    if p == 2 * n + 1:
        return "double_plus_one"
    return "many" if p >= 10 * n else "replace"


PLACEMENT_BRANCHES = ("empty", "far_only", "near_none", "far_none", "mixed", "equal", "extra_perm", "double", "double_plus_one",
                      "replace", "many")


def ref_rpn_points(c, t=None, call=0):
    """-> xyz (b, p, 3), intensity (b, p, 1), src_index (b, p), status (b,), rng_state after this call, info
    (call: the number of calls already made on the case's state).  info: per-frame branch, writes per slot, blocks per frame"""
    t = make_inputs(c) if t is None else t
    p, b = c["p"], len(c["frames"])
    seed, cn = int(t["state"][0]), int(t["state"][1]) + call
    xyz = np.zeros((b, p, 3), np.float32)
    inten = np.zeros((b, p, 1), np.float32)
    src = np.full((b, p), SENT_I, np.int32)
    status = np.zeros(b, np.int32)
    writes = np.zeros((b, p), np.int64)
    info = dict(branch=[], writes=writes, blocks=[], counts=[])
    total = t["total"]
    for f in range(b):
        s = min(max(int(t["offsets"][f]), 0), total)                    # rb_frame_range
        e = min(max(int(t["offsets"][f + 1]), s), total)
        pts = t["points"][s:e]
        cls, rect, _ = classify(pts, t["velo_to_rect"][f], t["p2"][f], t["wh"][f])
        near_i, far_i, kept_i = np.nonzero(cls == 1)[0], np.nonzero(cls == 2)[0], np.nonzero(cls != 0)[0]      # ranks in raw index order
        nn, nf, n = len(near_i), len(far_i), len(kept_i)
        info["branch"].append(placement_branch(p, nn, nf))
        info["blocks"].append(-(-(e - s) // THREADS))
        info["counts"].append((nn, nf))
        status[f] = (STATUS_EMPTY if n == 0 else 0) | (STATUS_TOO_MANY_FAR if (p < n and nf > p) else 0)

        def write(slots, rows):
            fx = rect[rows, 0].astype(np.float32)
            xyz[f, slots, 0] = -fx if t["flip"][f] else fx
            xyz[f, slots, 1] = rect[rows, 1].astype(np.float32)
            xyz[f, slots, 2] = rect[rows, 2].astype(np.float32)
            inten[f, slots, 0] = pts[rows, 3] - np.float32(0.5)
            src[f, slots] = rows
            np.add.at(writes[f], slots, 1)
        key = lambda purpose: rb_key(seed, cn, f, purpose)
        shuffle = lambda q: rb_apply(key(SHUFFLE), p, q)
        if n == 0:
            src[f] = -1
            writes[f] += 1
            continue
        if p < n:
            if nf > p:
                q = rb_apply(key(FAR), nf, np.arange(nf))
                write(shuffle(q[q < p]), far_i[q < p])
            else:
                m = p - nf
                if nn:
                    q = rb_apply(key(NEAR), nn, np.arange(nn))
                    write(shuffle(q[q < m]), near_i[q < m])
                write(shuffle(m + np.arange(nf)), far_i)
        else:
            write(shuffle(np.arange(n)), kept_i)
            extra = p - n
            if extra > 0 and p <= 2 * n:
                q = rb_apply(key(EXTRA), n, np.arange(n))
                write(shuffle(n + q[q < extra]), kept_i[q < extra])
            elif extra > 0:
                j = np.arange(extra)
                write(shuffle(n + j), kept_i[rb_index(key(DRAW), j, n)])
    return xyz, inten, src, status, state_after(t["state"], call + 1), info


# ================================================================================================ RPN labels
def _aligned_box_points(box, e):
    """points exactly on the faces of an axis-aligned box and of its enlarged box (where the face's coordinate is a float32), the
    other two coordinates at the box's centre"""
    x, y, z, l, w, h = (float(v) for v in box[:6])
    e = float(np.float32(e))
    cx, cy, cz = x, y - h / 2, z
    vals = {0: [], 1: [], 2: []}
    for grow, shift in ((0.0, 0.0), (2 * e, e)):
        hl, hw, hh = float(np.float32((l + grow) / 2.0)), float(np.float32((w + grow) / 2.0)), float(np.float32(h + grow))
        vals[0] += [x + hl, x - hl]
        vals[1] += [y + shift, y + shift - hh]
        vals[2] += [z - hw, z + hw]
    out = []
    for k in (0, 2, 1, 3):                  # interleaved: the first few already touch every axis and both boxes
        for d in (0, 1, 2):
            v = vals[d][k]
            if float(np.float32(v)) == v:
                pt = [cx, cy, cz]
                pt[d] = v
                out.append(pt)
    return np.array(out, np.float32).reshape(-1, 3)


def _labels_inputs(c):
    rng = np.random.default_rng(2000 + c["p"] + c["g"])
    b, p, g = c["b"], c["p"], c["g"]
    boxes = np.zeros((b, max(g, 0), 7), np.float32)
    classes = np.zeros((b, g), np.int32)
    xyz = np.zeros((b, p, 3), np.float32)
    e = float(np.float32(c["expand"]))
    for f, layout in enumerate(c["layout"]):
        if layout == "none":
            xyz[f] = rng.uniform(-3, 3, (p, 3)).astype(np.float32)
            continue
        if layout == "aligned":
            bx = np.array([[0.0, 0.0, 0.0, 2.0, 1.5, 1.0, 0.0]], np.float32)
            special = _aligned_box_points(bx[0], c["expand"])
        elif layout == "nested":
            # B (k = 0), A (k = 1), C (k = 2): B's ring reaches into A (ring first, inside later: A's class), C's ring too (inside
            # first, ring later: -1); B and C overlap A's enlarged box the other way round as well
            bx = np.array([[3.125, 0.0, 0.0, 2.0, 1.5, 1.0, 0.0], [0.0, 0.0, 0.0, 4.0, 2.0, 1.0, 0.0], [-3.125, 0.0, 0.0, 2.0, 1.5, 1.0, 0.0]], np.float32)
            special = np.concatenate([_aligned_box_points(q, c["expand"]) for q in bx] +
                                     [np.array([[2.0625, -0.5, 0.0], [-2.0625, -0.5, 0.0], [1.96875, -0.5, 0.25], [-1.96875, -0.5, 0.25],
                                                [2.15625, -0.5, 0.0], [-2.15625, -0.5, 0.0]], np.float32)], 0)
        else:
            cols = 16
            k = np.arange(g)
            bx = np.stack([-30 + 4.0 * (k % cols), rng.uniform(-0.5, 0.5, g), 5 + 3.0 * (k // cols), rng.uniform(1.5, 3.0, g),
                           rng.uniform(0.8, 2.0, g), rng.uniform(1.0, 2.0, g), rng.uniform(-np.pi, np.pi, g)], 1).astype(np.float32)
            special = np.zeros((0, 3), np.float32)
        boxes[f], classes[f] = bx, rng.integers(1, 4, g)
        special = special[:p]
        need = p - len(special)
        centre = bx[rng.integers(0, g, 4 * need + 16), :3].astype(np.float64)
        cand = (centre + np.stack([rng.uniform(-2.2, 2.2, len(centre)), rng.uniform(-2.4, 0.6, len(centre)), rng.uniform(-1.6, 1.6, len(centre))], 1)).astype(np.float32)
        if layout == "rotated":
            _, _, near = KN.rpn_labels(cand, bx.astype(np.float64), classes[f], e)
            _, _, near0 = KN.rpn_labels(cand, bx.astype(np.float64), classes[f], 0.0)
            cand = cand[np.minimum(near, near0) >= 1e-4]
        assert len(cand) >= need
        xyz[f] = np.concatenate([special, cand[:need]], 0)
    return dict(xyz=xyz, boxes=boxes, classes=classes, gt_count=np.array(c["counts"], np.int32))


def ref_rpn_labels(c, t=None):
    """-> label_cls (b, p) int32, label_reg (b, p, 7) float32, info (per-frame: points on a face, the two override orders)"""
    t = make_inputs(c) if t is None else t
    b, p, g = c["b"], c["p"], c["g"]
    e = float(np.float32(c["expand"]))
    cls, reg = np.zeros((b, p), np.int32), np.zeros((b, p, 7), np.float32)
    info = dict(on_face=0, ring_then_inside=0, inside_then_ring=0, ring=0, inside=0)
    for f in range(b):
        ng = min(max(int(t["gt_count"][f]), 0), g)
        if ng == 0:
            continue
        bx = t["boxes"][f, :ng].astype(np.float64)
        cls[f], reg[f], near = KN.rpn_labels(t["xyz"][f], bx, t["classes"][f, :ng], e)
        info["on_face"] += int((near == 0).sum())
        info["ring"] += int((cls[f] == -1).sum())
        info["inside"] += int((cls[f] > 0).sum())
        # the per-box events of every point, for the accounting of the override orders
        pts = t["xyz"][f].T.astype(np.float64)
        ext = bx.copy()
        ext[:, 3:6] += e * 2
        ext[:, 1] += e
        gc_, ec_ = KN.box_corners(bx), KN.box_corners(ext)
        ins = np.stack([KN.is_point_inside(pts, gc_[k].T)[0] for k in range(ng)])
        ring = np.stack([KN.is_point_inside(pts, ec_[k].T)[0] for k in range(ng)]) ^ ins
        for k in range(ng):
            info["ring_then_inside"] += int((ring[:k].any(0) & ins[k]).sum())
            info["inside_then_ring"] += int((ins[:k].any(0) & ring[k]).sum())
    return cls, reg, info


# ================================================================================================ image
def _image_inputs(c):
    rng = np.random.default_rng(3000 + c["src"][0] * 7 + c["src"][1])
    w, h = c["src"]
    imgs, offs, wh, off = [], [], [], 0
    valid = []
    for flip, jit, special in c["frames"]:
        fw, fh = (1, 1) if special == "pixel" else (w, h)
        im = rng.integers(0, 256, (fh, fw, 3)).astype(np.uint8)
        if special == "const":
            im[:] = (17, 130, 255)
        imgs.append(im)
        offs.append(off)
        off += im.size
        ok = True
        if special == "w0":
            fw, ok = 0, False
        if special == "h8193":
            fh, ok = 8193, False
        wh.append((fw, fh))
        valid.append(ok)
    buf = np.concatenate([im.reshape(-1) for im in imgs])
    for f, (_, _, special) in enumerate(c["frames"]):
        if special == "past":
            offs[f] = len(buf) - imgs[f].size + 3          # its last pixel ends 3 bytes past total_bytes
            valid[f] = False
    return dict(images=buf, frames=imgs, offsets=np.array(offs, np.int64), wh=np.array(wh, np.int32), valid=valid,
                flip=np.array([f[0] for f in c["frames"]], np.int32), jitter=np.array([f[1] for f in c["frames"]], np.int32),
                state=np.array(c["state"], np.int64), max_pixels=max([a * b_ for (a, b_), ok in zip(wh, valid) if ok] + [1]))


def noise_vector(e, v, normals):
    """sum_j sqrt(max(e_j, 0)) * v_ij * 0.1 * N_j in the kernel's order"""
    mag = normals * 0.1
    out = np.zeros(3)
    for i in range(3):
        acc = 0.0
        for j in range(3):
            acc = acc + math.sqrt(e[j] if e[j] > 0.0 else 0.0) * v[i][j] * mag[j]
        out[i] = acc
    return out


def ref_image(c, t=None, call=0, stats=None, noise=None):
    """-> image (b, H, W, 3) float32, noise (b, 3) fp64, rng_state after, info.  stats (b, 21): the e (9:12) and v (12:21) the noise
    vector is formed from (None: numpy.linalg.eigh of the covariance); noise (b, 3): the vector the jitter of the image applies
    (None: the one computed here)"""
    t = make_inputs(c) if t is None else t
    b = len(c["frames"])
    ow, oh = c["out"]
    seed, cn = int(t["state"][0]), int(t["state"][1]) + call
    image = np.zeros((b, oh, ow, 3), np.float32)
    nz = np.zeros((b, 3))
    info = dict(kind=[], blocks=[])
    for f in range(b):
        img = t["frames"][f]
        npx = img.shape[0] * img.shape[1]
        info["blocks"].append(-(-npx // IMG_PIX_PER_BLOCK))
        if not t["valid"][f]:
            info["kind"].append("invalid")
            continue
        jit = bool(t["jitter"][f])
        if jit and npx >= 2:
            if stats is None:
                e, v = np.linalg.eigh(KN.covariance(img))
            else:
                e, v = stats[f, 9:12], stats[f, 12:21].reshape(3, 3)
            nz[f] = noise_vector(e, v, image_normals(rb_key(seed, cn, f, NORMAL)))
        info["kind"].append(("jitter" if jit else "plain") + ("_flip" if t["flip"][f] else "") +
                            ("_one_pixel" if jit and npx < 2 else "") + ("_zero_cov" if jit and npx >= 2 and not np.ptp(img.reshape(-1, 3), axis=0).any() else ""))
        use = (nz[f] if noise is None else noise[f]) if jit else None
        image[f] = KN.image_sample(img, bool(t["flip"][f]), use, (oh, ow))
    return image, nz, state_after(t["state"], call + 1), info


# ================================================================================================ 3D IoU
def ref_bev_overlap(a, b):
    """float64 area of the intersection of the BEV rectangles of two (x, y, z, dx, dz, dy, ry) boxes: a Sutherland-Hodgman clip
    (corners as bev_iou's rotate_around_center)"""
    def corners(x):
        c, s = np.cos(x[6]), np.sin(x[6])
        out = []
        for dx, dz in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
            px, pz = dx * x[3] / 2, dz * x[4] / 2
            out.append((px * c + pz * s + x[0], -px * s + pz * c + x[2]))
        return out

    def clip(poly, p1, p2):
        out = []
        side = lambda q: (p2[0] - p1[0]) * (q[1] - p1[1]) - (p2[1] - p1[1]) * (q[0] - p1[0])
        for i in range(len(poly)):
            cur, prv = poly[i], poly[i - 1]
            sc, sp = side(cur), side(prv)
            if sc >= 0:
                if sp < 0:
                    t = sp / (sp - sc)
                    out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1])))
                out.append(cur)
            elif sp >= 0:
                t = sp / (sp - sc)
                out.append((prv[0] + t * (cur[0] - prv[0]), prv[1] + t * (cur[1] - prv[1])))
        return out

    def area(poly):
        return 0.5 * abs(sum(poly[i - 1][0] * poly[i][1] - poly[i][0] * poly[i - 1][1] for i in range(len(poly))))

    ca, cb = corners(a), corners(b)
    if area(ca) > 0 and sum(ca[i - 1][0] * ca[i][1] - ca[i][0] * ca[i - 1][1] for i in range(4)) < 0:
        ca = ca[::-1]
    if sum(cb[i - 1][0] * cb[i][1] - cb[i][0] * cb[i - 1][1] for i in range(4)) < 0:
        cb = cb[::-1]
    poly = list(ca)
    for i in range(4):
        if not poly:
            break
        poly = clip(poly, cb[i], cb[(i + 1) % 4])
    return area(poly) if len(poly) >= 3 else 0.0


def ref_iou3d(a, b):
    """float64 3D IoU: the BEV overlap of ref_bev_overlap times the height overlap, over max(va + vb - o3, 1e-7)"""
    inter = ref_bev_overlap(a, b)
    oh = max(min(a[1], b[1]) - max(a[1] - a[5], b[1] - b[5]), 0.0)
    o3 = inter * oh
    return o3 / max(a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - o3, 1e-7)


def bev_gap(a, b):
    """(n, g) separating-axis gap of the BEV rectangles in metres: > 0 exactly when they are disjoint (a lower bound of their
    distance), <= 0 when they overlap or touch"""
    def geom(x):
        x = np.asarray(x, np.float64).reshape(-1, 7)
        c, s = np.cos(x[:, 6]), np.sin(x[:, 6])
        d = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], np.float64)
        px, pz = d[None, :, 0] * x[:, None, 3] / 2, d[None, :, 1] * x[:, None, 4] / 2
        cor = np.stack([px * c[:, None] + pz * s[:, None] + x[:, None, 0], -px * s[:, None] + pz * c[:, None] + x[:, None, 2]], -1)
        axes = np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], 1)          # (n, 2 axes, 2)
        return cor, axes
    ca, xa = geom(a)
    cb, xb = geom(b)
    gap = np.full((len(ca), len(cb)), -np.inf)
    for axes, own in ((xa, True), (xb, False)):
        if own:
            pa = np.einsum("nkd,nad->nak", ca, axes)[:, None]                       # (n, 1, 2, 4)
            pb = np.einsum("gkd,nad->ngak", cb, axes)                               # (n, g, 2, 4)
        else:
            pa = np.einsum("nkd,gad->ngak", ca, axes)
            pb = np.einsum("gkd,gad->gak", cb, axes)[None]
        sep = np.maximum(pb.min(-1) - pa.max(-1), pa.min(-1) - pb.max(-1))          # (n, g, 2)
        gap = np.maximum(gap, sep.max(-1))
    return gap


def height_overlap(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.maximum(np.minimum(a[:, None, 1], b[None, :, 1]) - np.maximum(a[:, None, 1] - a[:, None, 5], b[None, :, 1] - b[None, :, 5]), 0.0)


def ref_iou3d_matrix(a, b):
    """(n, g) fp64 ref_iou3d of every pair -> (iou, gap, height overlap).  Pairs whose BEV rectangles a separating axis parts, or that do
    not overlap in height, are 0 without the clip (their intersection is empty)"""
    a, b = np.asarray(a, np.float64).reshape(-1, 7), np.asarray(b, np.float64)[:, :7].reshape(-1, 7)
    out = np.zeros((len(a), len(b)))
    if not len(a) or not len(b):
        return out, np.zeros_like(out), np.zeros_like(out)
    gap, oh = bev_gap(a, b), height_overlap(a, b)
    for i, j in np.argwhere((gap <= 0) & (oh > 0)):
        out[i, j] = ref_iou3d(a[i], b[j])
    return out, gap, oh


def f32_iou3d(oracle, a, b):
    """the float32 CPU form: the BEV overlap of the project's CPU oracle (an fp32 C restatement that never runs on the device), composed
    with the height overlap and the volumes in np.float32 in the order modules.box3d_iou writes them -> (n, g) float32"""
    a, b = np.asarray(a, np.float32).reshape(-1, 7), np.asarray(b, np.float32)[:, :7].reshape(-1, 7)
    if not len(a) or not len(b):
        return np.zeros((len(a), len(b)), np.float32)
    bev = lambda x: np.stack([x[:, 0] - x[:, 3] / np.float32(2), x[:, 2] - x[:, 4] / np.float32(2), x[:, 0] + x[:, 3] / np.float32(2),
                              x[:, 2] + x[:, 4] / np.float32(2), x[:, 6]], 1).astype(np.float32)
    ov, _ = oracle.compute_bev_iou(bev(a), bev(b))
    a_min, a_max = (a[:, 1] - a[:, 5])[:, None], a[:, 1][:, None]
    b_min, b_max = (b[:, 1] - b[:, 5])[None, :], b[:, 1][None, :]
    oh = np.maximum(np.minimum(a_max, b_max) - np.maximum(a_min, b_min), np.float32(0))
    o3 = ov * oh
    va, vb = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None, :]
    return (o3 / np.maximum(va + vb - o3, np.float32(1e-7))).astype(np.float32)


# ================================================================================================ RCNN targets
class ConditionError(AssertionError):
    pass


def _need(ok, what):
    if not ok:
        raise ConditionError(what)


def _thresholds(c):
    f32 = np.float32
    return f32(c["neg"][0]), f32(c["neg"][1]), min(f32(c["pos"][1]), f32(c["pos"][0]))


def check_iou_conditions(c, iou, gap, oh, props, gts):
    """the IoU conditions of the module docstring on one frame's (n, ng) fp64 matrix"""
    lo, hi, fg = (float(v) for v in _thresholds(c))
    n, ng = iou.shape
    if n == 0 or ng == 0:
        return
    _need(((iou == 0) | (iou >= DELTA)).all(), "a pair with 0 < IoU < DELTA")
    _need(((iou > 0) | (oh == 0) | (gap >= GAP)).all(), "a pair with IoU 0 closer than 1 cm")
    mx = iou.max(1)
    for thr in (lo, hi, fg):
        _need(((np.abs(mx - thr) >= DELTA) | (mx == 0)).all(), "a per-RoI maximum within DELTA of %g" % thr)   # an exact 0 is 0 on the device too
    for mat, boxes in ((iou, gts), (iou.T, props)):
        if mat.shape[1] < 2:
            continue
        order = np.argsort(-mat, axis=1, kind="stable")
        rows = np.arange(len(mat))
        best, second = mat[rows, order[:, 0]], mat[rows, order[:, 1]]
        same_box = (boxes[order[:, 0]] == boxes[order[:, 1]]).all(1)
        _need(((best - second > DELTA) | (best == 0) | same_box).all(), "best and second-best IoU within DELTA")


def _gt_grid(rng, ng, far):
    k = np.arange(ng)
    x, z = -28.0 + 8.0 * (k % 8), 8.0 + 6.0 * (k // 8)
    gt = np.stack([x + rng.uniform(-0.5, 0.5, ng), rng.uniform(1.4, 1.8, ng), z + rng.uniform(-0.5, 0.5, ng), rng.uniform(3.0, 4.5, ng),
                   rng.uniform(1.5, 2.0, ng), rng.uniform(1.4, 1.8, ng), rng.uniform(-np.pi, np.pi, ng), rng.integers(1, 4, ng)], 1)
    if far:
        gt[:, 0] += 500.0
    return gt.astype(np.float32)


def _candidate(rng, kind, gt):
    if kind == "easy" or not len(gt):
        return np.array([rng.uniform(-34, 34), rng.uniform(1.4, 1.8), rng.uniform(4, 104), rng.uniform(0.8, 4.5), rng.uniform(0.6, 2.0),
                         rng.uniform(1.2, 2.0), rng.uniform(-np.pi, np.pi)]).astype(np.float32)
    q = gt[rng.integers(0, len(gt)), :7].astype(np.float64)
    if kind == "fg":
        q = q + np.concatenate([rng.normal(0, 0.08, 3), np.zeros(3), rng.normal(0, 0.04, 1)])
        q[3:6] *= rng.uniform(0.95, 1.05, 3)
    elif kind == "hard":
        q = q + np.concatenate([rng.uniform(0.3, 1.3, 3) * rng.choice([-1, 1], 3) * (1, 0.2, 1), np.zeros(3), rng.normal(0, 0.3, 1)])
        q[3:6] *= rng.uniform(0.8, 1.2, 3)
    else:                                                   # high: the same footprint, no height overlap
        q[1] -= q[5] + rng.uniform(0.5, 3.0)
    return q.astype(np.float32)


def _frame_boxes(rng, c, fr):
    """(props (n, 7), gts (ng, 8)) float32 of one frame, every row checked against the row conditions as it is drawn"""
    lo, hi, fg = (float(v) for v in _thresholds(c))
    hi_kind = max(hi, 0.45)
    gts = _gt_grid(rng, fr["ng"], fr["far_gt"])
    if fr["twin_gt"] and fr["ng"] >= 2:
        gts[1] = gts[0]
    kinds = ["fg"] * fr["fg"] + ["hard"] * fr["hard"] + ["high"] * fr["high"] + ["easy"] * fr["easy"]
    props = np.zeros((fr["n"], 7), np.float32)
    for i, kind in enumerate(kinds):
        for _ in range(400):
            q = _candidate(rng, kind, gts)
            if fr["ng"] == 0:
                break
            row, gap, oh = ref_iou3d_matrix(q[None], gts)
            mx = row.max()
            srt = np.sort(row[0])[::-1]
            ok = ((row == 0) | (row >= DELTA)).all() and ((row > 0) | (oh == 0) | (gap >= GAP)).all()
            ok = ok and (mx == 0 or all(abs(mx - thr) >= DELTA for thr in (lo, hi, fg, 0.05, 0.45)))
            if len(srt) > 1 and srt[0] > 0 and not (fr["twin_gt"] and row[0, 0] == row[0, 1] == srt[0]):
                ok = ok and srt[0] - srt[1] > DELTA
            if kind == "fg":
                ok = ok and mx >= fg + 0.02
            elif kind == "hard":
                ok = ok and 0.05 < mx < hi_kind
            else:
                ok = ok and mx == 0
            if ok:
                break
        else:
            raise ConditionError("no %s proposal found" % kind)
        props[i] = q
    props = props[rng.permutation(len(props))] if len(props) else props
    if fr["twin_roi"] and fr["n"] >= 2:
        src = int(np.argmax(ref_iou3d_matrix(props, gts)[0].max(1))) if fr["ng"] else 0
        dst = (src + 1) % fr["n"]
        props[dst] = props[src]
    return props, gts


def _pack_targets(c, frames, boxes):
    b, m, g = c["b"], c["m"], c["g"]
    P, G = np.zeros((b, m, 7), np.float32), np.zeros((b, g, 8), np.float32)
    # padding rows hold huge boxes that would overlap everything: they must never be read
    P[:, :, 3:6], G[:, :, 3:6], G[:, :, 7] = 1000.0, 1000.0, 2.0
    pc, gc = np.zeros(b, np.int32), np.zeros(b, np.int32)
    for f, (fr, (props, gts)) in enumerate(zip(frames, boxes)):
        P[f, :len(props)], G[f, :len(gts)] = props, gts
        pc[f], gc[f] = fr["pc"], fr["gc"]
        assert min(max(fr["pc"], 0), m) == len(props) and min(max(fr["gc"], 0), g) == len(gts), (fr, m, g)
    return P, pc, G, gc


def _targets_inputs(c):
    frames = [dict(f) for f in c["frames"]]
    last = None
    for data_seed in range(16):
        rng = np.random.default_rng(4000 + 97 * data_seed + c["m"] * 3 + c["g"])
        try:
            boxes = [_frame_boxes(rng, c, fr) for fr in frames]
            P, pc, G, gc = _pack_targets(c, frames, boxes)
            mats = [ref_iou3d_matrix(p_, g_) for p_, g_ in boxes]
            for (p_, g_), (iou, gap, oh) in zip(boxes, mats):
                check_iou_conditions(c, iou, gap, oh, p_, g_[:, :7])
        except ConditionError as err:
            last = err
            continue
        t = dict(proposals=P, proposal_count=pc, gt=G, gt_count=gc, mats=mats, data_seed=data_seed)
        states = [c["state"]] if c["state"] is not None else [(s, 0) for s in range(32)]
        for st in states:
            t["state"] = np.array(st, np.int64)
            try:
                for call in range(c["calls"]):
                    ref_rcnn_targets(c, t, call=call, strict=True)
                return t
            except ConditionError as err:
                last = err
    raise AssertionError("%s: no seed satisfies the conditions: %s" % (case_id(c), last))


def aug_code(c):
    return AUG_METHODS[c["aug"]] if isinstance(c["aug"], str) else int(c["aug"])


def fg_per_image(c):
    return int(round(float(np.float32(c["fg_ratio"])) * c["r"]))           # nearbyint of the double product: half to even


def random_aug_box3d(method, key, f, s, base, box, dtype=np.float32):
    """one try's box from the float32 uniforms of (f, s, base + c); dtype float32: the kernel's expression tree in np.float32;
    float64: the same formula evaluated in fp64 (the measure of the 'normal' method's rounding) -> (box, the standard normals)"""
    T = dtype
    u = lambda k: T(tgt_uniform(key, f, s, base + k))
    pi = T(np.float32(math.pi))
    out = np.zeros(7, T)
    box = box.astype(T)
    normals = np.zeros(6)
    if method == 1:
        for d in range(3):
            out[d] = box[d] + (u(1 + d) - T(0.5))
        for d in range(3):
            out[3 + d] = box[3 + d] * ((u(4 + d) - T(0.5)) / (T(np.float32(0.5) / np.float32(0.15))) + T(1.0))
        out[6] = box[6] + (u(7) - T(0.5)) / T(np.float32(0.5) / (np.float32(math.pi) / np.float32(12.0)))
    elif method == 2:
        pos_r = [T(np.float32(v)) for v in (0.2, 0.3, 0.5, 0.8, 1.0)]
        hwl_r = [T(np.float32(v)) for v in (0.1, 0.15, 0.15, 0.15, 0.15)]
        ang_r = [T(np.float32(math.pi / k)) for k in (12, 12, 9, 6, 3)]
        row = int(tgt_index(tgt_uniform(key, f, s, base + 1), 5))
        for d in range(3):
            out[d] = box[d] + ((u(2 + d) - T(0.5)) / T(0.5)) * pos_r[row]
        for d in range(3):
            out[3 + d] = box[3 + d] * (((u(5 + d) - T(0.5)) / T(0.5)) * hwl_r[row] + T(1.0))
        out[6] = box[6] + ((u(8) - T(0.5)) / T(0.5)) * ang_r[row]
        normals[0] = row
    else:
        sigma = [T(np.float32(v)) for v in (0.3, 0.2, 0.3, 0.25, 0.15, 0.5)]
        for d in range(6):
            u1, u2 = T(1.0) - u(1 + 2 * d), u(2 + 2 * d)
            rad, ang = np.sqrt(T(-2.0) * np.log(u1)), np.cos(T(2.0) * pi * u2)
            out[d] = box[d] + sigma[d] * rad * ang
            normals[d] = float(rad) * float(ang)
        out[6] = box[6] + ((u(13) - T(0.5)) / T(0.5)) * pi / T(12.0)
    return out, normals


def ref_rcnn_targets(c, t=None, call=0, strict=False):
    """-> dict(rois (b, r, 7) f32, rois64 (the 'normal' method's fp64 evaluation), src (the proposals the slots started from), iou (b, r) fp64, gt_of_rois (b, r, 8) f32,
    stats (b, 4) int32, state (after this call), info).  strict: raise ConditionError where a jitter try's IoU lies within DELTA of
    fg_thresh"""
    t = make_inputs(c) if t is None else t
    b, m, g, r = c["b"], c["m"], c["g"], c["r"]
    lo, hi, fgt = _thresholds(c)
    aug, train = aug_code(c), c["train"]
    seed, cn = int(t["state"][0]), int(t["state"][1]) + call
    key = tgt_key(seed, cn)
    rois, rois64, src = np.zeros((b, r, 7), np.float32), np.zeros((b, r, 7)), np.zeros((b, r, 7), np.float32)
    iou_out, gt_out = np.zeros((b, r)), np.zeros((b, r, 8), np.float32)
    stats = np.zeros((b, 4), np.int32)
    info = dict(branch=[], mix=[], jitter=set(), dup_fg_slots=0, second_trip=set(), tries=0, max_normal=0.0, pairs=[], moved=np.zeros((b, r), bool),
                closest=np.inf)
    fpi = fg_per_image(c)
    hard_ratio = np.float32(c["hard_ratio"])
    for f in range(b):
        n, ng = min(max(int(t["proposal_count"][f]), 0), m), min(max(int(t["gt_count"][f]), 0), g)
        props, gts = t["proposals"][f, :n], t["gt"][f, :ng]
        iou = t["mats"][f][0]
        assert iou.shape == (n, ng)
        if n > THREADS:
            info["second_trip"].add("roi_loop")
        if ng > 0 and n > 0:
            s_max, s_arg = iou.max(1), iou.argmax(1)                # first argmax
            g_max, g_arg = iou.max(0), iou.argmax(0)
        else:
            s_max, s_arg = np.zeros(n), np.zeros(n, np.int64)
            g_max, g_arg = np.zeros(ng), np.zeros(ng, np.int64)
        fg = [i for i in range(n) if s_max[i] >= fgt] + [int(g_arg[j]) for j in range(ng) if g_max[j] > 0]
        easy = [i for i in range(n) if s_max[i] < lo]
        hard = [i for i in range(n) if not s_max[i] < lo and s_max[i] < hi]
        nfg, ne, nh = len(fg), len(easy), len(hard)

        def put(s, roi):
            if roi < 0:
                return
            rois[f, s] = src[f, s] = props[roi]
            rois64[f, s] = props[roi]
            if ng > 0:
                gt_out[f, s] = gts[s_arg[roi]]
            iou_out[f, s] = s_max[roi]
        if not train:
            for s in range(min(n, r)):
                put(s, s)
            stats[f] = (nfg, ne + nh, 0, 0)
            info["branch"].append("val" if n else "val_empty")
            continue
        fg_slots = bg_slots = 0
        if nfg > 0 and ne + nh > 0:
            fg_slots = min(fpi, nfg)
            for s in range(fg_slots):
                j = s + int(tgt_index(tgt_uniform(key, f, s, DRAW_PERM), nfg - s))
                fg[s], fg[j] = fg[j], fg[s]
            bg_slots = r - fg_slots
            branch = "fg+bg"
        elif nfg > 0:
            fg_slots, branch = r, "fg"
        elif ne + nh > 0:
            bg_slots, branch = r, "bg"
        else:
            branch = "neither"
        if n == 0:
            branch = "empty"
        info["branch"].append(branch)
        stats[f] = (nfg, ne + nh, fg_slots, bg_slots)
        if branch == "fg+bg":
            info["mix"].append(("below" if nfg < fpi else "above" if nfg > fpi else "equal") + ("_one" if nfg == 1 else ""))
            info["dup_fg_slots"] += fg_slots - len(set(fg[:fg_slots]))
        if bg_slots:
            info["mix"].append("hard+easy" if nh and ne else "hard_only" if nh else "easy_only")
        hard_slots = int(np.float32(bg_slots) * hard_ratio) if (nh > 0 and ne > 0) else (bg_slots if nh > 0 else 0)
        if r > THREADS:
            info["second_trip"].add("slot_loop")
        for s in range(r):
            if n == 0:
                continue
            if s < fg_slots:
                roi = fg[s] if branch == "fg+bg" else fg[int(tgt_index(tgt_uniform(key, f, s, DRAW_INDEX), nfg))]
                tries = FG_TRIES
            elif bg_slots > 0:
                q, u = s - fg_slots, tgt_uniform(key, f, s, DRAW_INDEX)
                roi = hard[int(tgt_index(u, nh))] if q < hard_slots else easy[int(tgt_index(u, ne))]
                tries = BG_TRIES
            else:
                roi, tries = int(tgt_index(tgt_uniform(key, f, s, DRAW_INDEX), n)), 0
            if aug == 0 or ng == 0:
                tries = 0
            put(s, roi)
            if tries == 0:
                if aug and branch != "neither":
                    info["jitter"].add("no_gt_no_try")
                continue
            # ---- the jitter loop
            box, gtb = props[roi], gts[s_arg[roi], :7]
            cur, cur64, tiou, k = box.copy(), box.astype(np.float64), 0.0, 0
            while tiou < fgt and k < tries:
                base = DRAW_JITTER + 16 * k
                if tgt_uniform(key, f, s, base) < np.float32(0.2):
                    cur, cur64 = box.copy(), box.astype(np.float64)
                    info["jitter"].add("kept")
                else:
                    cur, nrm = random_aug_box3d(aug, key, f, s, base, box)
                    cur64 = random_aug_box3d(aug, key, f, s, base, box, np.float64)[0] if aug == 3 else cur.astype(np.float64)
                    info["jitter"].add("moved")
                    if aug == 3:
                        info["max_normal"] = max(info["max_normal"], float(np.abs(nrm).max()))
                    if aug == 2:
                        info["jitter"].add("row%d" % int(nrm[0]))
                tiou = ref_iou3d(cur.astype(np.float64), gtb.astype(np.float64))
                info["closest"] = min(info["closest"], abs(tiou - float(fgt)))
                if strict:
                    _need(abs(tiou - float(fgt)) >= DELTA, "a jitter try within DELTA of fg_thresh")
                k += 1
                info["tries"] += 1
            info["jitter"].add(("fg_" if tries == FG_TRIES else "bg_") + ("stopped_early" if tiou >= fgt and k < tries else
                                                                           "stopped_last" if tiou >= fgt else "ran_out"))
            info["jitter"].add("method%d" % aug)
            info["moved"][f, s] = True
            rois[f, s], rois64[f, s], iou_out[f, s] = cur, cur64, tiou
            info["pairs"].append((cur.copy(), gtb.copy(), tiou))
    return dict(rois=rois, rois64=rois64, src=src, iou=iou_out, gt_of_rois=gt_out, stats=stats, state=state_after(t["state"], call + (1 if train else 0)),
                info=info)


def ref_iou_matrix(c, t=None):
    """hf_box3d_iou_matrix: (b, m, g) fp64, zeros in the padding (a row >= proposal_count[f] or a column >= gt_count[f])"""
    t = make_inputs(c) if t is None else t
    out = np.zeros((c["b"], c["m"], c["g"]))
    for f, (iou, _, _) in enumerate(t["mats"]):
        out[f, :iou.shape[0], :iou.shape[1]] = iou
    return out


def iou_bound(c, t, oracle, extra_pairs=()):
    """ELU_FACTOR x the largest error, over the case's pairs (the valid pairs of the matrix and the jitter loop's final pairs), of the
    float32 CPU form against the fp64 reference, floored at U -> (bound, the largest error)"""
    err = 0.0
    for f, (iou, _, _) in enumerate(t["mats"]):
        n, ng = iou.shape
        if n and ng:
            err = max(err, float(np.abs(f32_iou3d(oracle, t["proposals"][f, :n], t["gt"][f, :ng]).astype(np.float64) - iou).max()))
    for box, gtb, want in extra_pairs:
        err = max(err, abs(float(f32_iou3d(oracle, box[None], gtb[None])[0, 0]) - want))
    return ELU_FACTOR * max(err, U), err


_MAKERS = {"points": _points_inputs, "labels": _labels_inputs, "image": _image_inputs, "targets": _targets_inputs}
_CACHE = {}


def make_inputs(c):
    """the seeded inputs of a case (computed once per process; callers must not modify them)"""
    key = case_id(c)
    if key not in _CACHE:
        _CACHE[key] = _MAKERS[c["kind"]](c)
    return _CACHE[key]
