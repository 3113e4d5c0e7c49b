"""The row-gather family of csrc/row_gather.h through the C ABI, regime by regime (the case table, the restated launch rule, the
references and the scatter bound are in tests/row_gather_cases.py): ctypes on _lib.lib() with raw pointers, so that operands
one float past a 16-byte boundary can be handed over.  Forward results and gather-form gradients are compared bit for bit (as
int32) with the committed oracle, scatter gradients lie within the derived bound of the fp64 sum.  Every output is a slice of a
buffer filled with a NaN bit pattern: the guard floats around it and the columns beside a column slice must keep it."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_gather_cases as rc  # noqa: E402
from abi_harness import abi  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64                    # floats; a multiple of 4, so that the output keeps its alignment
_REF = {}                     # references are computed once per case and shared


def ref(kind, c, make):
    key = (kind, c["name"])
    if key not in _REF:
        _REF[key] = make()
        for a in (_REF[key] if isinstance(_REF[key], tuple) else (_REF[key],)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[key]


class Placed:
    """a host array on the device at a 16-byte boundary (off: one float past one); .p is the raw pointer"""

    def __init__(self, a, off=False):
        self.p = None
        if a is None:
            return
        flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.int32))
        o = 1 if off else 0
        self.buf = torch.empty(flat.numel() + 8, dtype=torch.int32, device=DEV)
        self.buf[o:o + flat.numel()].copy_(flat)
        assert self.buf.data_ptr() % 16 == 0
        self.p = ctypes.c_void_p(self.buf.data_ptr() + 4 * o)


class Out:
    """`count` output floats between two guards, everything filled with the sentinel bits"""

    def __init__(self, count, off=False):
        self.start, self.count = GUARD + (1 if off else 0), count
        self.buf = torch.full((self.start + count + GUARD,), rc.SENTINEL_BITS, dtype=torch.int32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.p = ctypes.c_void_p(self.buf.data_ptr() + 4 * self.start)

    def bits(self):
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert (host[:self.start] == rc.SENTINEL_BITS).all() and (host[self.start + self.count:] == rc.SENTINEL_BITS).all(), \
            "write outside the output"
        return host[self.start:self.start + self.count]

    def untouched(self):
        return bool((self.bits() == rc.SENTINEL_BITS).all())


def stream():
    return torch.cuda.current_stream().cuda_stream


def mk(rows):
    """(m, nsample) with m * nsample = rows"""
    return (rows // 3, 3) if rows % 3 == 0 else (rows, 1)


# ---------------------------------------------------------------- forward
def run_forward(c, points, idx, weight):
    _lib, L = abi()
    b, n, m, k, ch, width, col = (c[x] for x in ("b", "n", "m", "k", "c", "width", "col"))
    rows = m * k
    p, i, w = Placed(points, c["off"] == "points"), Placed(idx), Placed(weight)
    out = Out(b * rows * width, c["off"] == "out")
    if c["entry"] == "group_point":
        st = L.hf_group_point(b, n, ch, m, k, p.p, i.p, out.p, stream())
    elif c["entry"] == "group_point_into":
        st = L.hf_group_point_into(b, n, ch, m, k, width, col, p.p, i.p, out.p, stream())
    elif c["entry"] == "gather_point":
        st = L.hf_gather_point(b, n, rows, p.p, i.p, out.p, stream())
    else:
        st = L.hf_three_interpolate_cl(b, n, ch, rows, p.p, i.p, w.p, out.p, stream())
    _lib.check(st, c["name"])
    body = out.bits().reshape(b, rows, width)
    assert (body[:, :, :col] == rc.SENTINEL_BITS).all() and (body[:, :, col + ch:] == rc.SENTINEL_BITS).all(), \
        "write into the columns beside the slice"
    return body[:, :, col:col + ch]


@pytest.mark.parametrize("c", rc.FORWARD_CASES, ids=rc.case_id)
def test_forward_bit_equal(oracle_mod, c):
    points, idx, weight = ref("fwd_in", c, lambda: rc.forward_inputs(c))
    want = ref("fwd", c, lambda: rc.bits(rc.forward_oracle(oracle_mod, c, points, idx, weight)))
    got = run_forward(c, points, idx, weight)
    bad = int((got != want).sum())
    print("%s [%s]: %d of %d floats differ in bits" % (c["name"], rc.forward_regime(c)[0], bad, want.size))
    assert bad == 0
    if c["col"] or c["width"] != c["c"]:                         # the oracle has no strided form: the restatement, placed
        assert np.array_equal(got, rc.bits(rc.forward_restated(points, idx, weight)))


# ---------------------------------------------------------------- gradients
def inverse(L, nsrc, b, rows, n, idx):
    off = torch.empty((b, n + 1), dtype=torch.int32, device=DEV)
    ent = torch.empty((b, rows * nsrc), dtype=torch.int32, device=DEV)
    if nsrc == 3:
        st = L.hf_three_nn_inverse(b, rows, n, idx.p, off.data_ptr(), ent.data_ptr(), stream())
    else:
        st = L.hf_index_inverse(b, rows, n, idx.p, off.data_ptr(), ent.data_ptr(), stream())
    assert st == 0
    return off, ent


@pytest.mark.parametrize("c", rc.GATHER_GRAD_CASES, ids=rc.case_id)
def test_gather_form_gradient_bit_equal(oracle_mod, c):
    _lib, L = abi()
    idx, weight, wide = ref("grad_in", c, lambda: rc.grad_inputs(c))
    want = ref("gg", c, lambda: rc.bits(rc.grad_oracle(oracle_mod, c, idx, weight, wide)))
    b, n, rows, ch, ld, col = (c[x] for x in ("b", "n", "rows", "c", "ld", "col"))
    i, w, go = Placed(idx), Placed(weight), Placed(wide, c["off"])
    off, ent = inverse(L, c["nsrc"], b, rows, n, i)
    g = Out(b * n * ch)
    if c["nsrc"] == 1:
        m, k = mk(rows)
        st = L.hf_group_point_grad_gather(b, n, ch, m, k, ld, col, go.p, off.data_ptr(), ent.data_ptr(), g.p, stream())
    elif ld == ch:
        st = L.hf_three_interpolate_cl_grad_gather(b, rows, ch, n, go.p, w.p, off.data_ptr(), ent.data_ptr(), g.p, stream())
    else:
        st = L.hf_three_interpolate_concat_grad(b, rows, ch, n, ld, go.p, w.p, off.data_ptr(), ent.data_ptr(), g.p, stream())
    _lib.check(st, c["name"])
    got = g.bits().reshape(b, n, ch)
    bad = int((got != want).sum())
    print("%s [vec4=%s, block %d]: %d of %d floats differ in bits" % ((c["name"],) + rc.gather_grad_block(c)[::2] + (bad, want.size)))
    assert bad == 0
    assert (got[:, n - 1] == 0).all()                            # a target without entries is written as +0


@pytest.mark.parametrize("c", rc.SCATTER_CASES, ids=rc.case_id)
def test_scatter_gradient_within_bound(c):
    _lib, L = abi()
    idx, weight, wide = ref("grad_in", c, lambda: rc.grad_inputs(c))
    want, bound = ref("sc", c, lambda: rc.scatter_reference(c, idx, weight, wide))
    b, n, rows, ch, ld, col = (c[x] for x in ("b", "n", "rows", "c", "ld", "col"))
    m, k = mk(rows)
    i, w, go = Placed(idx), Placed(weight), Placed(wide)
    g = Out(b * n * ch)
    e = c["entry"]
    if e == "gather_point_grad":
        st = L.hf_gather_point_grad(b, n, rows, go.p, i.p, g.p, stream())
    elif e == "group_point_grad":
        st = L.hf_group_point_grad(b, n, ch, m, k, go.p, i.p, g.p, stream())
    elif e == "group_point_grad_from":
        st = L.hf_group_point_grad_from(b, n, ch, m, k, ld, col, go.p, i.p, g.p, stream())
    elif e == "group_concat_grad":
        st = L.hf_group_concat_grad(b, n, ch, m, k, ld, 1 if col == 0 else 0, go.p, i.p, g.p, stream())
    else:
        st = L.hf_three_interpolate_cl_grad(b, rows, ch, n, go.p, i.p, w.p, g.p, stream())
    _lib.check(st, c["name"])
    raw = g.bits().reshape(b, n, ch)
    got = raw.view(np.float32).astype(np.float64)
    diff = np.abs(got - want)
    ratio = float(np.max(diff[bound > 0] / bound[bound > 0]))
    print("%s: max |got - ref64| / bound = %.3g" % (c["name"], ratio))
    assert (diff <= bound).all()                                 # a NaN fails
    assert (raw[bound == 0] == 0).all()                          # unreferenced targets: the zero fill, untouched


# ---------------------------------------------------------------- empty shapes
def test_empty_shapes():
    """b = 0 launches nothing; no output rows: the forward writes nothing, the scatter gradients still zero-fill their target
    and the gather forms write it as zeros; three_interpolate_cl takes n = 0 unknown points the same way"""
    _lib, L = abi()
    z = Placed(np.zeros(64, np.float32))
    zi = Placed(np.zeros(64, np.int32))
    n, ch = 4, 3
    for b, rows in ((0, 5), (2, 0)):
        o = Out(64)
        assert L.hf_group_point(b, n, ch, rows, 1, z.p, zi.p, o.p, stream()) == _lib.HF_OK and o.untouched()
        assert L.hf_group_point_into(b, n, ch, rows, 1, 8, 4, z.p, zi.p, o.p, stream()) == _lib.HF_OK and o.untouched()
        assert L.hf_gather_point(b, n, rows, z.p, zi.p, o.p, stream()) == _lib.HF_OK and o.untouched()
        assert L.hf_three_interpolate_cl(b, n, ch, rows, z.p, zi.p, z.p, o.p, stream()) == _lib.HF_OK and o.untouched()
        calls = [lambda g: L.hf_gather_point_grad(b, n, rows, z.p, zi.p, g.p, stream()),
                 lambda g: L.hf_group_point_grad(b, n, ch, rows, 1, z.p, zi.p, g.p, stream()),
                 lambda g: L.hf_group_point_grad_from(b, n, ch, rows, 1, 8, 4, z.p, zi.p, g.p, stream()),
                 lambda g: L.hf_group_concat_grad(b, n, ch, rows, 1, 8, 0, z.p, zi.p, g.p, stream()),
                 lambda g: L.hf_three_interpolate_cl_grad(b, rows, ch, n, z.p, zi.p, z.p, g.p, stream()),
                 lambda g: L.hf_group_point_grad_gather(b, n, ch, rows, 1, 8, 4, z.p, zi.p, zi.p, g.p, stream()),
                 lambda g: L.hf_three_interpolate_cl_grad_gather(b, rows, ch, n, z.p, z.p, zi.p, zi.p, g.p, stream()),
                 lambda g: L.hf_three_interpolate_concat_grad(b, rows, ch, n, 8, z.p, z.p, zi.p, zi.p, g.p, stream())]
        for call in calls:
            g = Out(max(b, 1) * n * ch)
            assert call(g) == _lib.HF_OK
            if b == 0:
                assert g.untouched()
            else:
                assert (g.bits() == 0).all()
        off = Out(max(b, 1) * (n + 1))
        assert L.hf_index_inverse(b, rows, n, zi.p, off.p, zi.p, stream()) == _lib.HF_OK
        assert off.untouched() if b == 0 else (off.bits() == 0).all()
        off = Out(max(b, 1) * (n + 1))
        assert L.hf_three_nn_inverse(b, rows, n, zi.p, off.p, zi.p, stream()) == _lib.HF_OK
        assert off.untouched() if b == 0 else (off.bits() == 0).all()


# ---------------------------------------------------------------- inverse
def test_both_inverse_entries_agree_and_keep_their_limits():
    _lib, L = abi()
    b, rows, n = 2, 37, 41
    rng = np.random.default_rng(5)
    idx = rng.integers(0, n, (b, rows, 3)).astype(np.int32)
    idx[:, :, 0] = 7
    i = Placed(idx)
    results = []
    for nsrc_entry in (3, 1):
        off, ent = Out(b * (n + 1)), Out(b * rows * 3)
        if nsrc_entry == 3:
            st = L.hf_three_nn_inverse(b, rows, n, i.p, off.p, ent.p, stream())
        else:
            st = L.hf_index_inverse(b, rows * 3, n, i.p, off.p, ent.p, stream())
        assert st == _lib.HF_OK
        results.append((off.bits().reshape(b, n + 1), ent.bits().reshape(b, rows * 3)))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    for bb in range(b):
        flat = idx[bb].reshape(-1)
        assert np.array_equal(results[0][0][bb], np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=n))]))
        assert np.array_equal(results[0][1][bb], np.argsort(flat, kind="stable"))
    # limits: 8192 known points for three_nn_inverse, 19968 targets for index_inverse
    big = Placed(np.zeros(3, np.int32))
    off, ent = Out(19968 + 1), Out(3)
    assert L.hf_three_nn_inverse(1, 1, 8193, big.p, off.p, ent.p, stream()) == _lib.HF_EINVAL and off.untouched()
    assert L.hf_index_inverse(1, 3, 19969, big.p, off.p, ent.p, stream()) == _lib.HF_EINVAL and off.untouched()
    assert L.hf_three_nn_inverse(1, 1, 8192, big.p, off.p, ent.p, stream()) == _lib.HF_OK
    assert L.hf_index_inverse(1, 3, 8193, big.p, off.p, ent.p, stream()) == _lib.HF_OK
    o = off.bits()
    assert o[0] == 0 and (o[1:8194] == 3).all() and (ent.bits() == np.arange(3)).all()
    with pytest.raises(ValueError):
        from heterofusionrcnn_amd.interpolate import three_nn_inverse
        three_nn_inverse(torch.zeros((1, 1, 3), dtype=torch.int32, device=DEV), 8193)
