"""The fused X-apply + depthwise forward on channel pairs (packed f32 across two channels per lane, several rows in flight per
wave, X staged through LDS) against the CPU oracle: the same multiply-then-add sequence per output element, so bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heterofusionrcnn_amd", "csrc")


def _oracle_forward(x, fd, fts, idx, wd):
    """oracle.xconv_apply followed by oracle.depthwise_k on F_* = [F_delta | fts gathered through idx]"""
    import oracle
    b, p, k, _ = x.shape
    gathered = np.stack([fts[i][idx[i]] for i in range(b)])             # (b, p, k, c1)
    f = np.concatenate([fd, gathered], axis=-1)
    fx = oracle.xconv_apply(x.reshape(b * p, k, k), f.reshape(b * p, k, -1))
    return oracle.depthwise_k(fx, wd).reshape(b, p, -1)


def _case(b, n, p, k, c0, c1, m, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((b, p, k, k)).astype(np.float32)
    fd = rng.standard_normal((b, p, k, c0)).astype(np.float32)
    fts = rng.standard_normal((b, n, c1)).astype(np.float32)
    wd = rng.standard_normal((k, c0 + c1, m)).astype(np.float32)
    idx = rng.integers(0, n, (b, p, k)).astype(np.int32)
    return x, fd, fts, idx, wd


def _gather_forward(x, fd, fts, idx, wd):
    from heterofusionrcnn_amd import pointcnn as pc
    t = lambda a: torch.from_numpy(a).cuda()
    return pc.xconv_depthwise_gather(t(x), t(fd), t(fts), t(idx), t(wd)).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,c0,c1,m", [("dec5/dec4", 8, 64, 256, 1), ("dec3", 8, 128, 512, 1), ("enc0", 8, 64, 1, 4)])
def test_packed_forward_equals_oracle_at_layer_widths(name, k, c0, c1, m):
    """the channel widths of the rpn_multiclass layers (fewer rows than a full batch: the oracle runs on the host)"""
    x, fd, fts, idx, wd = _case(2, 1500, 1203, k, c0, c1, m, seed=c0 + c1 + m)
    assert np.array_equal(_gather_forward(x, fd, fts, idx, wd), _oracle_forward(x, fd, fts, idx, wd)), name


@pytest.mark.gpu
@pytest.mark.parametrize("k,c0,c1,m,p", [(8, 64, 1, 1, 37), (8, 64, 33, 1, 201), (8, 64, 65, 1, 99), (8, 128, 65, 2, 13),
                                          (8, 64, 33, 3, 77), (4, 64, 33, 1, 61), (4, 128, 64, 4, 9), (12, 64, 65, 1, 45),
                                          (12, 128, 40, 2, 5), (8, 192, 64, 1, 1)])
def test_packed_forward_equals_oracle_at_awkward_shapes(k, c0, c1, m, p):
    """odd c1 (a half-live last pair), rows per cloud not a multiple of the rows a block walks per trip, K = 4 / 12, M = 2 / 3,
    a 128-channel wave straddling the lifted / gathered split (c0 = 64, 192)"""
    x, fd, fts, idx, wd = _case(3, 50, p, k, c0, c1, m, seed=k * 1000 + c1 + p)
    assert np.array_equal(_gather_forward(x, fd, fts, idx, wd), _oracle_forward(x, fd, fts, idx, wd))


@pytest.mark.gpu
@pytest.mark.parametrize("c,m", [(1, 1), (65, 4), (320, 1), (33, 3), (128, 2)])
def test_packed_dense_forward_equals_oracle(c, m):
    """the non-gather form (hf_xconv_depthwise) shares the kernel: odd c reads and writes the pairs as single floats"""
    import oracle
    from heterofusionrcnn_amd import pointcnn as pc
    rng = np.random.default_rng(c + m)
    rows, k = 333, 8
    x = rng.standard_normal((rows, k, k)).astype(np.float32)
    f = rng.standard_normal((rows, k, c)).astype(np.float32)
    w = rng.standard_normal((k, c, m)).astype(np.float32)
    got = pc.xconv_depthwise(torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(w).cuda()).cpu().numpy()
    assert np.array_equal(got.reshape(rows, -1), oracle.depthwise_k(oracle.xconv_apply(x, f), w))


@pytest.mark.gpu
def test_staged_and_rebuilt_table_gradients_at_dec5_size():
    """at the last decoder layer's size (8 clouds x 16384 rows, c0 64, c1 256): the table gradient staged in the workspace
    and the one rebuilt per table row are equal, and so are the other gradients; grad_wd to 1e-5 relative"""
    from heterofusionrcnn_amd import pointcnn as pc
    from heterofusionrcnn_amd.grouping import index_inverse
    torch.manual_seed(11)
    b, n, p, k, c0, c1 = 8, 16384, 16384, 8, 64, 256
    x = torch.randn(b, p, k, k, device="cuda", requires_grad=True)
    fd = torch.randn(b, p, k, c0, device="cuda", requires_grad=True)
    fts = torch.randn(b, n, c1, device="cuda", requires_grad=True)
    wd = torch.randn(k, c0 + c1, 1, device="cuda", requires_grad=True)
    idx = torch.randint(0, n, (b, p, k), device="cuda", dtype=torch.int32)
    inv = index_inverse(idx, n)
    go = torch.randn(b, p, c0 + c1, device="cuda")
    outs, grads = [], []
    for use_ws in (True, False):
        out = pc.xconv_depthwise_gather(x, fd, fts, idx, wd, inv, use_workspace=use_ws)
        outs.append(out.detach())
        grads.append(torch.autograd.grad(out, (x, fd, fts, wd), go))
    assert torch.equal(outs[0], outs[1])
    for a, r, name in zip(grads[0][:3], grads[1][:3], ("x", "f_delta", "fts")):
        assert torch.equal(a, r), name
    assert float((grads[0][3] - grads[1][3]).abs().max()) <= 1e-5 * float(grads[1][3].abs().max())


def test_packed_forward_kernels_keep_coefficients_in_registers(tmp_path):
    """compiled with the Makefile's flags: every xconv_dw_fwd_kernel instantiation has no SGPR / VGPR spills and no scratch
    (the X coefficients come from LDS broadcasts, not SGPR pairs)"""
    asm = tmp_path / "xconv.s"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-ffp-contract=off",
                    "-std=c++17", "-I" + os.path.join(CSRC, "..", "..", "include"), "--cuda-device-only", "-S",
                    os.path.join(CSRC, "xconv.hip"), "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    found = 0
    for blk in re.split(r"\n\s*- \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "xconv_dw_fwd_kernel" not in name:
            continue
        found += 1
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
        assert field("sgpr_spill_count") == 0 and field("vgpr_spill_count") == 0, name
        assert field("private_segment_fixed_size") == 0, name
        assert field("vgpr_count") <= 256, name
    assert found == 8 * 2 * 2      # (K, M) pairs x gather form x paired accesses
