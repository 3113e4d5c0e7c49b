"""Case table and references of the ORDERED image-feature gradients (hf_project_gather_grad_ordered, hf_crop_and_resize_grad_ordered;
csrc/ordered_scatter.h).  tests/test_ordered_grad_cases_cpu.py checks this module on any machine, tests/test_ordered_grad_abi.py runs the
cases on the GPU through the C ABI, tests/test_deterministic_image.py goes through the Python layer.  A plain helper module: the
references come from the contract of include/hfops.h, never from the kernels.

The contract.  E entries in a fixed order, each with a target row key[e] of the (b*h*w, c) map or none, and a term of c floats;
grad_img[t] = the terms of { e : key[e] == t } added in ascending e, in fp32, from +0.0f, one rounding per add.  `entries_*` restate
(valid, key, term) of the two ops as arrays, `sequential` is the loop

    for e in range(E):
        if valid[e]: g[key[e]] += term[e]

on a zero-filled float32 array, and `sequential(..., descending=True)` the same loop from the last entry to the first (the CPU test
shows that the order is visible in the bits of these cases, so a kernel that adds in another order fails them).

project_gather: entry e = bb*p + point, valid when pix [u,v] is inside [0,w) x [0,h), key = (bb*h + v)*w + u, term = grad_out[e].
crop_and_resize: entry e = ((r*crop_h + i)*crop_w + j)*4 + tap, taps tl, tr, bl, br; validity, pixels and ly / lx from
roi_image_cases.samples (the fp32 restatement of the sample coordinates); terms in np.float32, one rounding per operation:
dtop = (1-ly) g, dbot = ly g, tl = (1-lx) dtop, tr = lx dtop, bl = (1-lx) dbot, br = lx dbot.

grad_out of the project cases is sign * 2^k * U(1,2) with k in [-12, 12] and a few -0.0: sums of three or more such terms depend on
their order.  Pixels are drawn and written into `pix` directly (the ABI test needs no projection); about one value in twenty is -1, w
or h (outside).

Against the atomic entries: a pixel with at most two entries has the same bits either way (0 + a + b, fp32 addition commutes; the
one exception, a lone -0.0, gives +0 both ways); elsewhere both lie within (k + 4) 2^-24 sum|g| of the fp64 sum, the bound that
roi_image_cases.ref_backward derives for a sum in any order (`bound_any_order` restates it for the project cases, whose terms carry
no rounding of their own)."""
import functools
import zlib

import numpy as np

import roi_image_cases as rc

U = 2.0 ** -24

# name: (b, p, h, w, c)
PROJECT_CASES = {
    "scalar_c3": (2, 200, 3, 5, 3),          # up to ~18 entries a pixel: lists either side of the 16 a thread sorts alone; scalar width
    "step64_c32": (1, 70, 1, 1, 32),         # one list crossing a 64-lane step
    "chunk1024_c4": (1, 1300, 1, 1, 4),      # one list crossing a 1024-entry chunk
    "straddle_c5": (3, 600, 7, 1300, 5),     # lists around multiples of 1024 in the flat pixel index; a frame of zeros; several scan chunks
    "wide_c40": (2, 64, 4, 6, 40),           # c > 32 and not a power of two
    "global_sort_c2": (1, 5000, 1, 1, 2),    # one list beyond the 4096 ids that are sorted in LDS
    "empty_p": (2, 0, 4, 6, 4),
    "empty_b": (0, 5, 4, 6, 4),
}
# ten pixels of straddle_c5 by flat index (bb*h + v)*w + u, frames 0 and 2; frame 1 has every point outside the image
HOT_PIXELS = {0: (1023, 1024, 4095, 4096, 4097, 8191, 8192), 2: (20479, 20480, 24576)}
ZERO_FRAME = 1


def _rng(name, salt):
    return np.random.default_rng(zlib.crc32(("ordered/%s/%s" % (name, salt)).encode()))


def order_sensitive_values(rng, shape):
    """sign * 2^k * U(1,2), k in [-12, 12], about one value in fifty -0.0"""
    v = rng.choice([-1.0, 1.0], shape) * np.exp2(rng.integers(-12, 13, shape)) * rng.uniform(1.0, 2.0, shape)
    v = v.astype(np.float32)
    v[rng.random(shape) < 0.02] = np.float32(-0.0)
    return v


@functools.lru_cache(maxsize=None)
def make_project(name):
    """-> dict go (b,p,c) float32, pix (b,p,2) int32 [u,v]; read-only"""
    b, p, h, w, c = PROJECT_CASES[name]
    rng = _rng(name, "inputs")
    u, v = rng.integers(0, w, (b, p)), rng.integers(0, h, (b, p))
    if name == "straddle_c5":
        for bb in range(b):
            if bb == ZERO_FRAME:
                u[bb], v[bb] = rng.choice([-1, w], p), rng.integers(-1, h + 1, p)
                continue
            hot = np.array(HOT_PIXELS[bb]) - bb * h * w
            pick = hot[rng.integers(0, len(hot), p // 2)]
            u[bb, :p // 2], v[bb, :p // 2] = pick % w, pick // w
            order = rng.permutation(p)
            u[bb], v[bb] = u[bb, order], v[bb, order]
    if name in ("scalar_c3", "straddle_c5", "wide_c40"):
        out = rng.random((b, p)) < 0.05
        u = np.where(out & (rng.random((b, p)) < 0.5), rng.choice([-1, w], (b, p)), u)
        v = np.where(out & (u >= 0) & (u < w), rng.choice([-1, h], (b, p)), v)
    pix = np.stack([u, v], axis=-1).astype(np.int32).reshape(b, p, 2)
    go = order_sensitive_values(rng, (b, p, c))
    for a in (pix, go):
        a.setflags(write=False)
    return dict(go=go, pix=pix)


def entries_project(name, go=None):
    """-> (targets, valid (E), key (E) int64, term (E,c) float32)"""
    b, p, h, w, c = PROJECT_CASES[name]
    t = make_project(name)
    go = t["go"] if go is None else go
    u, v = t["pix"][..., 0].astype(np.int64), t["pix"][..., 1].astype(np.int64)
    valid = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    key = (np.arange(b)[:, None] * h + v) * w + u
    return b * h * w, valid.reshape(-1), np.where(valid, key, 0).reshape(-1), go.reshape(b * p, c)


def entries_crop(shape, boxes, ind, go):
    """-> (targets, valid (E), key (E) int64, term (E,c) float32) of crop_and_resize_grad on an image of `shape`"""
    b, h, w, c = shape
    n, ch, cw, _ = go.shape
    s = rc.samples(b, h, w, ch, cw, boxes, ind)
    one = np.float32(1)
    ly, lx = s["ly"].astype(np.float32)[:, :, None, None], s["lx"].astype(np.float32)[:, None, :, None]     # exact: fp32 values
    assert np.array_equal(ly.astype(np.float64)[:, :, 0, 0], s["ly"]) and np.array_equal(lx.astype(np.float64)[:, 0, :, 0], s["lx"])
    g = go.astype(np.float32)
    dtop, dbot = (one - ly) * g, ly * g
    term = np.stack([(one - lx) * dtop, lx * dtop, (one - lx) * dbot, lx * dbot], axis=3)                     # (n, ch, cw, 4, c)
    assert term.dtype == np.float32
    full = (n, ch, cw)
    y0, yb = (np.broadcast_to(a[:, :, None], full) for a in (s["y0"], s["yb"]))
    x0, xb = (np.broadcast_to(a[:, None, :], full) for a in (s["x0"], s["xb"]))
    bi = np.broadcast_to(s["bi"][:, None, None], full)
    key = np.stack([(bi * h + yy) * w + xx for yy, xx in ((y0, x0), (y0, xb), (yb, x0), (yb, xb))], axis=3)  # (n, ch, cw, 4)
    valid = np.broadcast_to(s["ok"][..., None], key.shape)
    return b * h * w, valid.reshape(-1), np.where(valid, key, 0).reshape(-1), term.reshape(-1, c)


def sequential(targets, valid, key, term, descending=False):
    """the loop of the contract on a zero-filled float32 (targets, c) array"""
    g = np.zeros((targets, term.shape[1]), np.float32)
    order = np.flatnonzero(valid)
    for e in (order[::-1] if descending else order):
        g[key[e]] += term[e]
    return g


def counts(targets, valid, key):
    return np.bincount(key[valid], minlength=targets)


def bound_any_order(targets, valid, key, term):
    """-> (fp64 sum (targets,c), (k + 4) 2^-24 sum|term|): the bound of roi_image_cases.ref_backward for a sum in any order"""
    want, mag = np.zeros((targets, term.shape[1])), np.zeros((targets, term.shape[1]))
    np.add.at(want, key[valid], term[valid].astype(np.float64))
    np.add.at(mag, key[valid], np.abs(term[valid]).astype(np.float64))
    return want, (counts(targets, valid, key)[:, None] + 4) * U * mag


@functools.lru_cache(maxsize=None)
def project_reference(name):
    """-> dict grad (b,h,w,c) float32, k (b,h,w), want64, bound; computed once, read-only"""
    b, p, h, w, c = PROJECT_CASES[name]
    targets, valid, key, term = entries_project(name)
    want, bound = bound_any_order(targets, valid, key, term)
    r = dict(grad=sequential(targets, valid, key, term).reshape(b, h, w, c), k=counts(targets, valid, key).reshape(b, h, w),
             want64=want.reshape(b, h, w, c), bound=bound.reshape(b, h, w, c))
    for a in r.values():
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def crop_reference(name, bad_ind=False):
    """-> dict grad (b,h,w,c) float32, k (b,h,w) of a roi_image_cases.CROP_CASES entry; computed once, read-only"""
    t = rc.make_inputs(name, bad_ind)
    targets, valid, key, term = entries_crop(t["img"].shape, t["boxes"], t["ind"], t["go"])
    r = dict(grad=sequential(targets, valid, key, term).reshape(t["img"].shape), k=counts(targets, valid, key).reshape(t["img"].shape[:3]))
    for a in r.values():
        a.setflags(write=False)
    return r
