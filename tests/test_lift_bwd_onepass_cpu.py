"""The one-pass form of the lifting chain's first-layer weight gradient (csrc/lift_bwd.hip), on the host: the closed form with the
eleven sums is autograd's dW0, and an emulation of the kernel's arithmetic -- fp32 sums inside a workgroup, fp64 across workgroups,
the formula in fp64 -- stays within gemm_cases.lift_bwd_bounds for a zero-mean dz1 and for a mean-dominated one (the input that
would expose cancellation between A_d and the two correction terms).  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

EPS = 1e-3
ROWS, C0, C1 = 131072, 64, 64      # the size of the issue's own emulation: 1024 tiles, one per workgroup


def _inputs(dz_mean):
    g = torch.Generator().manual_seed(20251)
    x3 = torch.randn(ROWS, 3, generator=g) * 0.5
    w0 = torch.randn(C0, 3, generator=g)
    gamma0, beta0 = torch.rand(C0, generator=g) + 0.5, torch.rand(C0, generator=g) - 0.5
    w1 = torch.randn(C1, C0, generator=g) * 0.3
    dz1 = torch.randn(ROWS, C1, generator=g) + dz_mean
    return x3, w0, gamma0, beta0, w1, dz1


def eleven_sums(x3, w0, mean, invstd, dy0, dtype, block_rows=None):
    """sum v, sum v xhat, A_d, B_d, C_d per channel: (11, c0) in fp64.  dtype = the arithmetic of the elementwise terms and of the sums
    inside a block of block_rows rows (None: one block); blocks are added in fp64"""
    x, w = x3.to(dtype), w0.to(dtype)
    z0 = (x[:, 0:1] * w[:, 0] + x[:, 1:2] * w[:, 1]) + x[:, 2:3] * w[:, 2]          # lift_z's order
    e = torch.where(z0 > 0, z0, torch.exp(z0) - 1.0)
    s = torch.where(z0 > 0, torch.ones_like(z0), torch.exp(z0))
    xhat = (e - mean.to(dtype)) * invstd.to(dtype)
    v = dy0.to(dtype)
    terms = [v, v * xhat]
    sx = [s * x[:, d:d + 1] for d in range(3)]
    terms += [v * sx[d] for d in range(3)] + sx + [xhat * sx[d] for d in range(3)]
    block_rows = block_rows or x.shape[0]
    out = []
    for t in terms:
        blocks = [b.sum(0, dtype=dtype).double() for b in t.split(block_rows)]
        out.append(torch.stack(blocks).sum(0))
    return torch.stack(out)


def closed_form(S, gamma0, invstd, rows):
    """dW0 (c0, 3) in fp64 from the eleven fp64 sums"""
    a = gamma0.double() * invstd.double()
    return torch.stack([a * (S[2 + d] - S[0] / rows * S[5 + d] - S[1] / rows * S[8 + d]) for d in range(3)], 1)


def test_closed_form_is_autograds_dw0_in_fp64():
    x3, w0, gamma0, beta0, w1, dz1 = _inputs(0.0)
    x3, dz1 = x3[:4099], dz1[:4099]
    _, gg0, gb0, gw0, mean, invstd = gc.ref_lift_bwd_autograd(x3, w0, gamma0, beta0, w1, dz1, EPS)
    S = eleven_sums(x3, w0, mean, invstd, dz1.double() @ w1.double(), torch.float64)
    got = closed_form(S, gamma0, invstd, x3.shape[0])
    assert float((S[0] - gb0).abs().max()) <= 1e-12 * float(gb0.abs().max())
    assert float((S[1] - gg0).abs().max()) <= 1e-12 * float(gg0.abs().max())
    assert float((got - gw0).abs().max()) <= 1e-12 * float(gw0.abs().max())


@pytest.mark.parametrize("dz_mean", [0.0, 5.0], ids=["zero_mean", "mean_five_times_the_spread"])
def test_fp32_in_block_fp64_across_blocks_stays_within_the_bounds(dz_mean):
    x3, w0, gamma0, beta0, w1, dz1 = _inputs(dz_mean)
    gw1, gg0, gb0, gw0, mean, invstd = gc.ref_lift_bwd_autograd(x3, w0, gamma0, beta0, w1, dz1, EPS)
    m32, i32 = mean.float(), invstd.float()                     # the kernel is given the statistics rounded to fp32
    dy0 = (dz1.double() @ w1.double()).float()                  # the MFMA chain's own c1 u D error is part of the bound, not of this test
    S = eleven_sums(x3, w0, m32, i32, dy0, torch.float32, block_rows=gc.FWD_ROWS)
    got = closed_form(S, gamma0, i32, ROWS).float()
    b = gc.lift_bwd_bounds(x3, w0, [gamma0, beta0, mean, invstd], w1, dz1, 16 * gc.tiles_per_workgroup(ROWS, gc.cdiv(C0, 32)) + 4, 1)
    for name, g, ref, bound in (("dbeta0", S[0].float(), gb0, b["d_dbeta"]), ("dgamma0", S[1].float(), gg0, b["d_dgamma"]),
                                ("grad_w0", got, gw0, b["d_w0"])):
        diff = (g.double() - ref).abs()
        print("%s: max |emulation - ref64| / bound = %.3g, relative to the largest element %.3g" % (
            name, float((diff / bound).max()), float(diff.max() / ref.abs().max())))
        assert bool((diff <= bound).all()), name
