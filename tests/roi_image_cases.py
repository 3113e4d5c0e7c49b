"""Case table, references and bounds of the RoI image kernels of csrc/roi_image.hip (hf_roi_image_boxes, hf_crop_and_resize,
hf_crop_and_resize_grad).  tests/test_roi_image_cases_cpu.py checks this module on any machine, tests/test_roi_image_abi.py runs the
cases on the GPU through the C ABI, tests/test_roi_image.py goes through the Python layer.  A plain helper module: the references
come from the formulas of include/hfops.h, never from the kernels.

Crop reference.  The sample coordinates are restated in np.float32, one rounding per operation in the order the header gives
(in_y = y1 (h-1) + i ((y2-y1) (h-1) / (crop_h-1)), or 0.5 (y1+y2) (h-1) for crop_h == 1): IEEE fp32 on both sides gives the same
bits, so the in-range decision, floor and ceil are those of the kernel, and ly = in_y - floor(in_y) is exact in fp32: the weights
are common to both sides.  The interpolation from those coordinates is fp64.

Forward bound: |got - ref| <= 2^-19 max|img|.  top and bot carry at most 5 roundings each on magnitudes <= 2 max|img|, the last
lerp brings the total to <= 20 2^-24 max|img|; 32 2^-24 leaves a margin.

Backward reference: an fp64 scatter-add with the weights above.  Bound per element: (k + 4) 2^-24 G, k the number of contributions
the reference scattered to the element (four per in-range sample: when floor == ceil two of them land on one element and both
count), G the sum of their |g|, unweighted: four roundings per contribution and k - 1 for a sum in any order (the atomics).  It holds
for (1-lx)((1-ly) g) and for a g - g l form; a bound weighted by the bilinear weights would not hold for the latter.  k = 0: exactly 0.

Boxes of a case: uniform in [-0.2, 1.2] (seeded by the case name), with forced rows in front, as many as fit:
  [nan, 0.1, 0.5, inf]       not finite: every comparison fails, the row is all extrapolation and adds nothing to the gradient
  [0, 0, 1, 1]               the last sample may or may not round past h - 1: the restatement decides
  zero area, inverted        all samples on one point; coordinates running backwards
  lattice                    y1 = x1 = 0 and a step of one pixel where the image is large enough (crop 1: the centre on pixel 0):
                             floor == ceil
  two identical boxes        on the same frame: every element they touch has k >= 2
  wholly outside             beyond 1.2 on both axes
box_ind is uniform in [0, b); bad_ind=True appends one row with box_ind -1 and one with b (the ABI test).

Grid.  Both crop kernels are grid-stride loops of 256-thread blocks, at most 2048 blocks (grid_for in hf_common.h): a lane takes a
second item past 524 288 items.  The forward has n crop_h crop_w c / 4 items (vector path), the gradient n crop_h crop_w c: the
300-box case takes a second trip in neither (117 600 / 470 400 items), the 1400-box case "rounds" in both (548 800 / 2 195 200).

Box projection: boxes drawn as tests/test_rcnn.py::test_project_boxes_and_geometry_helpers draws them (depth 8-40 m: no corner
behind the camera), two different P2 matrices in one batch; reference: modules.box_3d_to_box_8co in float64 on the host, times P2,
divided by depth, min / max; bounds as there: pixels rtol 1e-4 atol 1e-2, normalised rtol 1e-4 atol 1e-4."""
import functools
import zlib

import numpy as np

U = 2.0 ** -24
THREADS, MAX_BLOCKS = 256, 2048
FWD_BOUND = 2.0 ** -19

# name: (b, h, w, c, (crop_h, crop_w), n, extrapolation)
CROP_CASES = {
    "scalar_c3": (2, 9, 13, 3, (4, 4), 40, -3.5),
    "vec_c32": (2, 9, 13, 32, (7, 7), 40, 0.0),
    "crop1_c5": (3, 24, 40, 5, (1, 1), 60, 0.0),
    "many_c32": (3, 24, 40, 32, (7, 7), 300, 0.0),
    "tiny": (1, 2, 2, 4, (2, 2), 10, 0.0),
    "one_pixel": (1, 1, 1, 4, (3, 3), 6, 0.0),
    "rect_c8": (2, 9, 13, 8, (3, 5), 12, 0.0),        # crop_h != crop_w: through the ABI only
    "rounds_c32": (2, 24, 40, 32, (7, 7), 1400, 0.0),
    "empty": (2, 9, 13, 4, (7, 7), 0, 0.0),
}
SQUARE = tuple(k for k, v in CROP_CASES.items() if v[4][0] == v[4][1])

BOX_CASES = {"one": (1, 1), "two_frames": (2, 5), "three_frames": (3, 67), "empty": (2, 0)}
IMAGE_HW = (360, 1200)
P2_A = np.array([[721.5, 0, 609.6, 44.9], [0, 721.5, 172.9, 0.2], [0, 0, 1, 0.003]], np.float32)
P2_B = np.array([[707.0, 0, 604.1, 45.8], [0, 707.0, 180.5, -0.35], [0, 0, 1, 0.0049]], np.float32)
PX_TOL, NORM_TOL = dict(rtol=1e-4, atol=1e-2), dict(rtol=1e-4, atol=1e-4)


def dims(name):
    b, h, w, c, (ch, cw), n, extrap = CROP_CASES[name]
    return dict(b=b, h=h, w=w, c=c, ch=ch, cw=cw, n=n, extrap=extrap)


def _rng(name, salt):
    return np.random.default_rng(zlib.crc32(("%s/%s" % (name, salt)).encode()))


def forced_rows(d):
    """the rows in front of every case's boxes, as (box, frame or None)"""
    end = lambda crop, size: 0.0 if crop == 1 else (min(1.0, (crop - 1) / (size - 1)) if size > 1 else 1.0)
    lat_y, lat_x = end(d["ch"], d["h"]), end(d["cw"], d["w"])
    return [([np.nan, 0.1, 0.5, np.inf], None), ([0, 0, 1, 1], None), ([0.3, 0.6, 0.3, 0.6], None), ([0.9, 0.8, 0.1, 0.2], None),
            ([0, 0, lat_y, lat_x], None), ([0.2, 0.1, 0.7, 0.8], 0), ([0.2, 0.1, 0.7, 0.8], 0), ([1.3, 1.3, 1.8, 1.9], None)]


@functools.lru_cache(maxsize=None)
def make_inputs(name, bad_ind=False):
    """-> dict img (b,h,w,c), boxes (n,4), ind (n) int32, go (n,ch,cw,c): float32 arrays, read-only"""
    d = dims(name)
    rng = _rng(name, "inputs")
    img = rng.standard_normal((d["b"], d["h"], d["w"], d["c"])).astype(np.float32)
    n = d["n"]
    boxes = rng.uniform(-0.2, 1.2, (n, 4)).astype(np.float32)
    ind = rng.integers(0, d["b"], n).astype(np.int32)
    for r, (box, frame) in enumerate(forced_rows(d)[:n]):
        boxes[r] = box
        if frame is not None:
            ind[r] = frame
    if bad_ind and n:
        boxes = np.concatenate([boxes, np.array([[0, 0, 1, 1]], np.float32), boxes[-1:]])
        ind = np.concatenate([ind, np.array([-1, d["b"]], np.int32)])
    go = rng.standard_normal((boxes.shape[0], d["ch"], d["cw"], d["c"])).astype(np.float32)
    out = dict(img=img, boxes=boxes, ind=ind, go=go)
    for a in out.values():
        a.setflags(write=False)
    return out


def finite_rows(boxes):
    return np.isfinite(boxes).all(axis=1)


def _axis(a1, a2, crop, size):
    """fp32 sample coordinates of one axis, (n, crop)"""
    sm1 = np.float32(size - 1)
    if crop > 1:
        step = (a2 - a1) * sm1 / np.float32(crop - 1)
        return (a1 * sm1)[:, None] + np.arange(crop, dtype=np.float32)[None] * step[:, None]
    return (np.float32(0.5) * (a1 + a2) * sm1)[:, None]


def samples(b, h, w, ch, cw, boxes, ind):
    """the fp32 restatement: -> dict ok (n,ch,cw) bool; y0, yb (n,ch), x0, xb (n,cw) int64 (0 where the coordinate is out of
    range); ly (n,ch), lx (n,cw) float64"""
    boxes = np.asarray(boxes, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ys = _axis(boxes[:, 0], boxes[:, 2], ch, h)
        xs = _axis(boxes[:, 1], boxes[:, 3], cw, w)
        assert ys.dtype == np.float32 and xs.dtype == np.float32
        oky = (ys >= 0) & (ys <= np.float32(h - 1))           # a NaN fails both
        okx = (xs >= 0) & (xs <= np.float32(w - 1))
    okb = (ind >= 0) & (ind < b)
    ok = oky[:, :, None] & okx[:, None, :] & okb[:, None, None]
    ys, xs = np.where(oky, ys, np.float32(0)), np.where(okx, xs, np.float32(0))
    y0f, x0f = np.floor(ys), np.floor(xs)
    ly, lx = ys - y0f, xs - x0f
    assert ly.dtype == np.float32 and lx.dtype == np.float32
    return dict(ok=ok, y0=y0f.astype(np.int64), yb=np.ceil(ys).astype(np.int64), x0=x0f.astype(np.int64),
                xb=np.ceil(xs).astype(np.int64), ly=ly.astype(np.float64), lx=lx.astype(np.float64),
                bi=np.where(okb, ind, 0).astype(np.int64))


def ref_forward(img, boxes, ind, ch, cw, extrap):
    """fp64 (n,ch,cw,c) from the fp32 coordinates"""
    b, h, w, c = img.shape
    s = samples(b, h, w, ch, cw, boxes, ind)
    img64 = img.astype(np.float64)
    bi = s["bi"][:, None, None]
    g = lambda yy, xx: img64[bi, yy[:, :, None], xx[:, None, :]]
    lx, ly = s["lx"][:, None, :, None], s["ly"][:, :, None, None]
    tl, tr, bl, br = g(s["y0"], s["x0"]), g(s["y0"], s["xb"]), g(s["yb"], s["x0"]), g(s["yb"], s["xb"])
    top = tl + (tr - tl) * lx
    bot = bl + (br - bl) * lx
    return np.where(s["ok"][..., None], top + (bot - top) * ly, np.float64(extrap))


def ref_backward(shape, boxes, ind, go):
    """-> (grad_img fp64 (b,h,w,c), bound (b,h,w,c), k (b,h,w) contributions per element)"""
    b, h, w, c = shape
    n, ch, cw, _ = go.shape
    s = samples(b, h, w, ch, cw, boxes, ind)
    grad = np.zeros((b * h * w, c), np.float64)
    mag = np.zeros((b * h * w, c), np.float64)
    k = np.zeros(b * h * w, np.int64)
    sel = s["ok"]
    go64 = go.astype(np.float64)[sel]                            # (S, c)
    bi = np.broadcast_to(s["bi"][:, None, None], sel.shape)[sel]
    full = lambda a, axis: np.broadcast_to(a[:, :, None] if axis == "y" else a[:, None, :], sel.shape)[sel]
    ly, lx = full(s["ly"], "y"), full(s["lx"], "x")
    for yy, wy in ((full(s["y0"], "y"), 1.0 - ly), (full(s["yb"], "y"), ly)):
        for xx, wx in ((full(s["x0"], "x"), 1.0 - lx), (full(s["xb"], "x"), lx)):
            flat = (bi * h + yy) * w + xx
            np.add.at(grad, flat, (wy * wx)[:, None] * go64)
            np.add.at(mag, flat, np.abs(go64))
            np.add.at(k, flat, 1)
    bound = (k[:, None] + 4) * U * mag
    return grad.reshape(shape), bound.reshape(shape), k.reshape(b, h, w)


@functools.lru_cache(maxsize=None)
def reference(name, bad_ind=False):
    """the references of a case, computed once: out, grad, grad_bound, k, ok, fwd_bound"""
    d, t = dims(name), make_inputs(name, bad_ind)
    out = ref_forward(t["img"], t["boxes"], t["ind"], d["ch"], d["cw"], d["extrap"])
    grad, bound, k = ref_backward(t["img"].shape, t["boxes"], t["ind"], t["go"])
    ok = samples(d["b"], d["h"], d["w"], d["ch"], d["cw"], t["boxes"], t["ind"])["ok"]
    r = dict(out=out, grad=grad, grad_bound=bound, k=k, ok=ok, fwd_bound=FWD_BOUND * float(np.abs(t["img"]).max()))
    for a in r.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r


def grid_rounds(name):
    """(forward items, gradient items) / (MAX_BLOCKS * THREADS), rounded up: 2 = a lane takes a second item"""
    d = dims(name)
    smp = d["n"] * d["ch"] * d["cw"]
    per = MAX_BLOCKS * THREADS
    fwd = smp * (d["c"] // 4 if d["c"] % 4 == 0 else d["c"])
    return -(-fwd // per), -(-smp * d["c"] // per)


# ---------------------------------------------------------------------------------------------------------- box projection
@functools.lru_cache(maxsize=None)
def make_boxes3d(name):
    """-> (boxes3d (b,n,7), calib (b,3,4)) float32"""
    b, n = BOX_CASES[name]
    rng = _rng(name, "boxes3d")
    boxes = np.concatenate([rng.uniform(-10, 10, (b, n, 1)), rng.uniform(0, 2, (b, n, 1)), rng.uniform(8, 40, (b, n, 1)),
                            rng.uniform(1, 4, (b, n, 3)), rng.uniform(-3, 3, (b, n, 1))], -1).astype(np.float32)
    calib = np.stack([P2_A if f % 2 == 0 else P2_B for f in range(b)])
    boxes.setflags(write=False)
    calib.setflags(write=False)
    return boxes, calib


def ref_boxes(boxes, calib, image_hw):
    """fp64: -> (pixels (b*n,4) [x1,y1,x2,y2], normalised by [w,h,w,h])"""
    import torch

    from heterofusionrcnn_amd.modules import box_3d_to_box_8co
    b, n, _ = boxes.shape
    c8 = box_3d_to_box_8co(torch.from_numpy(boxes.reshape(-1, 7).astype(np.float64))).numpy().reshape(b, n, 3, 8)
    assert c8.dtype == np.float64
    hom = np.concatenate([c8, np.ones((b, n, 1, 8))], axis=2)                  # (b, n, 4, 8)
    pix = np.einsum("bij,bnjk->bnik", calib.astype(np.float64), hom)
    uv = pix[:, :, :2] / pix[:, :, 2:3]
    px = np.concatenate([uv.min(axis=3), uv.max(axis=3)], axis=2).reshape(b * n, 4)
    h, w = image_hw
    return px, px / np.array([w, h, w, h], np.float64)
