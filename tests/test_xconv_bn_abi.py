"""csrc/xconv_bn.hip through the C ABI: the X-Conv gather kernels with the lifting BatchNorm folded in against the two-launch route
they replace, ctypes on _lib.lib() with no Python routing in between.

The reference is the library's own present route on the same device buffers: hf_bn_relu_fwd_eval(z1, mode 2) into a buffer f, then
hf_xconv_depthwise_gather(f) / hf_xconv_depthwise_gather_grad(f, with a workspace).  The folded kernels use that route's arithmetic
element for element, so out, grad_x, grad_f, grad_wd and grad_fts must be the SAME BITS: a mismatch is a bug, not rounding.  dgamma and
dbeta are new sums in another order than hf_bn_relu_bwd's; they are held to fp64 NumPy / torch sums of the kernel's own grad_f with the
bound form tests/bn_cases.py derives for the bn_bwd sums (ref_bn_bwd: gamma(chain + 3) sum |dh| X + the ELU term + the cast), `chain` =
the fp32 additions on the longest path into one block's partial.  Inputs are seeded normals / uniforms (no integers: every order of adds
rounds differently), outputs are sentinel-guarded slices, inputs lie between NaN bands (tests/abi_harness.py's In / Out).

Shapes.  B = 2 clouds of n_src = 50 table rows and P = 37 points: 74 rows.
  forward   xdw_pair_grid gives 19 blocks of rows_per_block = 4 (the last one 2): a block trip covers 8 rows (4 waves x kXcRows = 2), so
            in EVERY trip the second row of each wave lies past the block's end, is clamped to the block's last row and not stored, and
            in the last block waves 2 and 3 have no row at all; cloud 1 starts at row 37, inside block 9 (rows 36 .. 39).
  backward  xdw_bwd_grid's floor of 32 rows per block gives 3 blocks of 32, 32 and 10 rows: the BatchNorm partials of three blocks meet
            in the finalize kernel, the last block is ragged (waves 2 and 3 walk 2 rows, waves 0 and 1 walk 3).
  tall      B = 2, P = 4200 (8400 rows) at (8, 1), c0 = 128, c1 = 64: the forward launcher gives rows_per_block = 9 (one full trip and a
            second one in which only wave 0 has a row; 934 blocks, the last one 3 rows), the backward one 263 blocks of 32 rows, the last
            one 16.  P is sized from those two numbers, which the test reads back from the workspace query.
c0 = 64: a forward wave (128 channels) straddles the lifted / gathered split at lane 32; c0 = 128: it does not.  c1 = 1 makes c odd: V2 =
false loads and a dead upper half in the last pair; c1 = 64 and 66 are the V2 = true forms, 66 with one live pair in the last chunk."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_cases as bc  # noqa: E402
import xconv_cases as xc  # noqa: E402
from abi_harness import SENTINEL, Arena, In, Out, abi, call, parity_report, within  # noqa: E402
from xconv_runs import check_argument_limits  # noqa: E402

pytestmark = pytest.mark.gpu

KM = ((8, 1), (8, 2), (8, 4))
B, N_SRC, P = 2, 50, 37
TALL = dict(k=8, m=1, c0=128, c1=64, b=2, n=N_SRC, p=4200)
CASES = [dict(k=k, m=m, c0=c0, c1=c1, b=B, n=N_SRC, p=P) for (k, m) in KM for c0 in (64, 128) for c1 in (1, 64, 66)] + [TALL]
OUTPUTS = ("out", "x", "f", "wd", "fts", "dgamma", "dbeta")
DEV = "cuda"
parity_report = parity_report("XCONV_BN_PARITY_OUT", "hf_xconv_depthwise_gather_bn")      # the source of profiles/xconv_bn_parity.md


def case_id(c):
    return "k%dm%d-c%d+%d-b%dp%dn%d" % (c["k"], c["m"], c["c0"], c["c1"], c["b"], c["p"], c["n"])


def make_inputs(c):
    rng = np.random.default_rng(xc._seed(dict(c, kind="bwd", family="round", regime="bn", gather=True, off=())))
    k, m, c0, c1, b, n, p = (c[key] for key in ("k", "m", "c0", "c1", "b", "n", "p"))
    rows = b * p
    normal = lambda *s: rng.standard_normal(s, np.float32)
    t = dict(x=normal(rows, k, k), z1=normal(rows * k, c0), fts=normal(b * n, c1), wd=normal(k, c0 + c1, m), go=normal(rows, (c0 + c1) * m),
             gamma=rng.uniform(0.5, 1.5, c0).astype(np.float32), beta=(0.1 * normal(c0)).astype(np.float32),
             mean=(0.1 * normal(c0)).astype(np.float32), invstd=rng.uniform(0.5, 2.0, c0).astype(np.float32),
             idx=rng.integers(0, n, (b, p, k)).astype(np.int32))
    t["offsets"], t["entries"] = xc.index_inverse(t["idx"], n)
    return t


class Device:
    """the case's inputs on the device, shared by the two routes and by the repeated calls"""

    def __init__(self, c, t):
        self.c, self.t = c, t
        for name in ("x", "z1", "fts", "wd", "go", "gamma", "beta", "mean", "invstd", "idx", "offsets", "entries"):
            setattr(self, name, In(DEV, t[name]))


def dims(c):
    return c["b"], c["n"], c["p"], c["k"], c["c0"], c["c1"], c["m"]


def sizes(c):
    b, n, p, k, c0, c1, m = dims(c)
    rows, ch = b * p, c0 + c1
    return dict(out=rows * ch * m, x=rows * k * k, f=rows * k * c0, wd=k * ch * m, fts=b * n * c1, dgamma=c0, dbeta=c0)


def run_old(d):
    """hf_bn_relu_fwd_eval into a buffer, then the unfolded pair of entries (the gradient with its workspace)"""
    _lib, L = abi()
    sp = _lib.stream_ptr()
    c = d.c
    b, n, p, k, c0, c1, m = dims(c)
    sz = sizes(c)
    a = Arena(DEV)
    f = Out(a, sz["f"])
    call(L.hf_bn_relu_fwd_eval(b * p * k, c0, d.z1.p, d.gamma.p, d.beta.p, d.mean.p, d.invstd.p, 2, f.p, sp), "hf_bn_relu_fwd_eval")
    g = {name: Out(a, sz[name]) for name in ("out", "x", "f", "wd", "fts")}
    call(L.hf_xconv_depthwise_gather(b, n, p, k, c0, c1, m, d.x.p, f.p, d.fts.p, d.idx.p, d.wd.p, g["out"].p, sp), "hf_xconv_depthwise_gather")
    nbytes = L.hf_xconv_depthwise_gather_grad_workspace(b, p, k, c0, c1, m)
    ws = Out(a, nbytes // 4, fill=SENTINEL)
    call(L.hf_xconv_depthwise_gather_grad(b, n, p, k, c0, c1, m, d.x.p, f.p, d.fts.p, d.idx.p, d.wd.p, d.go.p, d.offsets.p, d.entries.p, g["x"].p,
                                          g["f"].p, g["fts"].p, g["wd"].p, ws.p, nbytes, sp), "hf_xconv_depthwise_gather_grad")
    a.check()
    return {name: o.view for name, o in g.items()}


def run_new(d):
    _lib, L = abi()
    sp = _lib.stream_ptr()
    c = d.c
    b, n, p, k, c0, c1, m = dims(c)
    sz = sizes(c)
    a = Arena(DEV)
    g = {name: Out(a, sz[name]) for name in OUTPUTS}
    call(L.hf_xconv_depthwise_gather_bn(b, n, p, k, c0, c1, m, d.x.p, d.z1.p, d.gamma.p, d.beta.p, d.mean.p, d.invstd.p, d.fts.p, d.idx.p,
                                        d.wd.p, g["out"].p, sp), "hf_xconv_depthwise_gather_bn")
    nbytes = L.hf_xconv_depthwise_gather_bn_grad_workspace(b, p, k, c0, c1, m)
    ws = Out(a, nbytes // 4, fill=SENTINEL)
    call(L.hf_xconv_depthwise_gather_bn_grad(b, n, p, k, c0, c1, m, d.x.p, d.z1.p, d.gamma.p, d.beta.p, d.mean.p, d.invstd.p, d.fts.p, d.idx.p,
                                             d.wd.p, d.go.p, d.offsets.p, d.entries.p, g["x"].p, g["f"].p, g["fts"].p, g["wd"].p, g["dgamma"].p,
                                             g["dbeta"].p, ws.p, nbytes, sp), "hf_xconv_depthwise_gather_bn_grad")
    a.check()
    return {name: o.view for name, o in g.items()}


def bn_chain(c):
    """fp32 additions on the longest path into one block's partial: a lane adds the K values of each of its rows (a wave walks every
    fourth row of the block), then the four waves meet one after the other; the blocks are added in double"""
    _, _, rpb = xc.xdw_bwd_grid(c["b"] * c["p"], c["c0"] + c["c1"])
    return xc.cdiv(rpb, xc.WAVES) * c["k"] + xc.WAVES - 1


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_folded_entries_against_the_two_launch_route(c):
    t = make_inputs(c)
    d = Device(c, t)
    old, new = run_old(d), run_new(d)
    for name in ("out", "x", "f", "wd", "fts"):
        same = torch.equal(old[name], new[name])
        differ = 0 if same else int((old[name] != new[name]).sum())
        print("%s: %d of %d elements differ from the two-launch route" % (name, differ, new[name].numel()))
        assert same, "grad_%s / out: %d of %d elements are not the bits of the two-launch route" % (name, differ, new[name].numel())
    # dgamma / dbeta: fp64 sums of the kernel's own grad_f (dh) against elu(z1) normalised in fp64
    c0 = c["c0"]
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    r = bc.ref_bn_bwd(tt(t["z1"]), new["f"].cpu().reshape(-1, c0), tt(t["gamma"]), tt(t["beta"]), tt(t["mean"]), tt(t["invstd"]), 2, bn_chain(c))
    within(new["dbeta"].cpu(), r["dbeta"], r["d_dbeta"], "hf_xconv_depthwise_gather_bn_grad.dbeta", case_id(c))
    within(new["dgamma"].cpu(), r["dgamma"], r["d_dgamma"], "hf_xconv_depthwise_gather_bn_grad.dgamma", case_id(c))
    # no atomics anywhere: two more calls, the same bits in every output
    for _ in range(2):
        again = run_new(d)
        for name in OUTPUTS:
            assert torch.equal(new[name], again[name]), "%s: %d of %d elements differ between two calls" % (
                name, int((new[name] != again[name]).sum()), new[name].numel())


def test_the_launchers_give_the_geometry_the_shapes_were_sized_for():
    """rows_per_block of both launchers, read back from the library: the backward grid is the number of partial rows in the workspace"""
    _, L = abi()
    for c, fwd, bwd in ((CASES[0], (19, 4, 2), (3, 32, 10)), (TALL, (934, 9, 3), (263, 32, 16))):
        b, n, p, k, c0, c1, m = dims(c)
        rows, ch = b * p, c0 + c1
        gx, _, rpb = xc.xdw_pair_grid(rows, ch)
        assert (gx, rpb, rows - (gx - 1) * rpb) == fwd
        gx, _, rpb = xc.xdw_bwd_grid(rows, ch)
        assert (gx, rpb, rows - (gx - 1) * rpb) == bwd and gx >= 3
        base = (L.hf_xconv_depthwise_gather_grad_workspace(b, p, k, c0, c1, m) + 255) // 256 * 256
        assert base == (xc.gather_grad_workspace(b, p, k, c0, c1, m) + 255) // 256 * 256
        assert L.hf_xconv_depthwise_gather_bn_grad_workspace(b, p, k, c0, c1, m) == base + 4 * gx * 2 * c0


def test_one_past_each_argument_limit_is_refused():
    check_argument_limits()
