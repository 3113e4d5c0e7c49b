"""The feature table's gradient of the gather-form X-Conv (hf_xconv_depthwise_gather_grad): rebuilt per table row from grad_out by
xconv_dw_bwd_fts_kernel (channel pairs, several table rows and list entries in flight per wave) instead of staged as a
rows x K x c1 block and summed by hf_group_point_grad_gather.  Same multiply / add sequence per element, so bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "heterofusionrcnn_amd", "csrc")


def _random_idx(rng, b, n, p, k):
    return rng.integers(0, n, (b, p, k)).astype(np.int32)


def _ladder_idx(rng, n, p, k):
    """one cloud's table: row i is named i % 11 times (lists of length 0, 1, ..., 10: empty, single, and lengths that are not
    a multiple of the entries a wave takes per trip), the slots in random order"""
    flat, i = [], 0
    while len(flat) < p * k:
        flat += [i % n] * (i % 11)
        i += 1
    flat = np.asarray(flat[:p * k], np.int32)
    return flat[rng.permutation(p * k)].reshape(p, k)


def _check(b, n, p, k, c0, c1, m, seed, idx=None, misalign=False):
    """default call (workspace given: the library picks the route), use_workspace=False (rebuilt per table row) and the
    materialised reference (concat_group + xconv_depthwise) agree"""
    from heterofusionrcnn_amd import pointcnn as pc
    from heterofusionrcnn_amd.grouping import concat_group, index_inverse
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    dev = "cuda"
    x = torch.randn(b, p, k, k, device=dev, requires_grad=True)
    fd = torch.randn(b, p, k, c0, device=dev, requires_grad=True)
    fts = torch.randn(b, n, c1, device=dev, requires_grad=True)
    wd = torch.randn(k, c0 + c1, m, device=dev, requires_grad=True)
    if idx is None:
        idx = _random_idx(rng, b, n, p, k)
    idx = torch.from_numpy(np.ascontiguousarray(idx)).to(dev)
    inv = index_inverse(idx, n)
    width = (c0 + c1) * m
    if misalign:      # grad_out starts one float past a 16-byte boundary: the single-float form of the kernel
        go = torch.randn(b * p * width + 1, device=dev)[1:].view(b, p, width)
        assert go.data_ptr() % 16 != 0
    else:
        go = torch.randn(b, p, width, device=dev)
    ref = pc.xconv_depthwise(x, concat_group(fd, fts, idx, inv), wd)
    g_ref = torch.autograd.grad(ref, (x, fd, fts, wd), go)
    for use_ws in (True, False):
        out = pc.xconv_depthwise_gather(x, fd, fts, idx, wd, inv, use_workspace=use_ws)
        g = torch.autograd.grad(out, (x, fd, fts, wd), go)
        assert torch.equal(out, ref), use_ws
        for a, r, name in zip(g[:3], g_ref[:3], ("x", "f_delta", "fts")):
            assert torch.equal(a, r), (name, use_ws)
        assert float((g[3] - g_ref[3]).abs().max()) <= 1e-5 * float(g_ref[3].abs().max()), use_ws
    return g_ref[2], idx


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,p,c0,c1,m", [("enc1", 1500, 400, 64, 256, 1), ("enc2", 800, 210, 64, 256, 2), ("enc3", 500, 130, 128, 512, 2),
                                               ("enc4", 256, 64, 256, 1024, 1), ("dec0", 64, 64, 256, 1280, 1), ("dec1", 64, 256, 256, 1024, 1),
                                               ("dec2", 256, 1024, 256, 1024, 1), ("dec3", 300, 1203, 128, 512, 1),
                                               ("dec4", 400, 1600, 64, 256, 1), ("dec5", 1500, 1500, 64, 256, 1)])
def test_table_gradient_at_layer_widths(name, n, p, c0, c1, m):
    """the channel widths and (K, M) of the ten gather layers of rpn_multiclass, with fewer rows"""
    _check(3, n, p, 8, c0, c1, m, seed=c0 + c1 + m + p)


@pytest.mark.gpu
def test_table_gradient_at_dec4_size():
    """8 clouds x 16384 queries onto 4096 table rows (c0 64, c1 256): lists of about 32 entries, several trips per table row"""
    g, idx = _check(8, 4096, 16384, 8, 64, 256, 1, seed=4)
    counts = torch.bincount(idx.reshape(8, -1)[0].long(), minlength=4096)
    assert 24 <= float(counts.float().mean()) <= 40 and int(counts.max()) > 40


@pytest.mark.gpu
@pytest.mark.parametrize("k,c0,c1,m,n,p", [(8, 64, 33, 1, 50, 61), (8, 64, 1, 1, 50, 37), (8, 64, 1, 4, 70, 70), (8, 64, 40, 1, 90, 45),
                                            (8, 64, 66, 1, 50, 99), (8, 128, 66, 2, 31, 13), (8, 64, 33, 3, 50, 77), (8, 64, 96, 3, 40, 77),
                                            (8, 128, 64, 4, 50, 9), (8, 64, 260, 1, 33, 100), (4, 64, 33, 1, 50, 61), (4, 128, 64, 4, 20, 90),
                                            (4, 64, 256, 1, 128, 512), (12, 64, 65, 1, 50, 45), (12, 128, 40, 2, 17, 5), (12, 64, 128, 2, 64, 128),
                                            (12, 64, 512, 1, 64, 64), (8, 192, 64, 1, 5, 1)])
def test_table_gradient_at_awkward_shapes(k, c0, c1, m, n, p):
    """c1 odd, 1, below one wave's channels, not a multiple of 4, past one wave's channels by a few; K = 4 and 12; M = 2, 3, 4;
    rows per cloud different from the table's rows; random lists (lengths 0, 1, 2, ...)"""
    _check(3, n, p, k, c0, c1, m, seed=k * 1000 + c1 * 7 + p + m)


@pytest.mark.gpu
@pytest.mark.parametrize("k,c1,m", [(8, 256, 1), (8, 33, 1), (12, 64, 2), (4, 32, 4)])
def test_table_gradient_with_skewed_and_empty_lists(k, c1, m):
    """cloud 0: one table row named by every slot, every other row by none; cloud 1: lists of 0 .. 10 entries; cloud 2: random,
    with the last table row of the last cloud unnamed (its gradient row is written as zeros, not left as it was)"""
    b, n, p = 3, 300, 203
    rng = np.random.default_rng(k + c1 + m)
    idx = _random_idx(rng, b, n, p, k)
    idx[0] = 7
    idx[1] = _ladder_idx(rng, n, p, k)
    idx[2][idx[2] == n - 1] = 0
    g, _ = _check(b, n, p, k, 64, c1, m, seed=k * c1 + m, idx=idx)
    assert not g[2, n - 1].any() and not g[0, 8:].any() and not g[0, :7].any() and g[0, 7].any()
    lens = np.bincount(idx[1].reshape(-1), minlength=n)
    assert {0, 1, 3, 5, 9, 10} <= set(lens.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("c1,m", [(256, 1), (64, 2)])
def test_table_gradient_with_grad_out_off_a_16_byte_boundary(c1, m):
    _check(2, 100, 150, 8, 64, c1, m, seed=c1 + m, misalign=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,b,n,p,k,c0,c1,m,staged", [
    ("enc2 at 8 frames: lists of 2, m 2, 64 MiB", 8, 4096, 1024, 8, 64, 256, 2, True),
    ("enc4 at 8 frames: lists of 2, m 1, 16 MiB", 8, 256, 64, 8, 256, 1024, 1, True),
    ("RCNN first layer, fewer RoIs: k 4, m 4, lists of 4, 34 MiB", 8, 512, 512, 4, 128, 544, 4, True),
    ("RCNN last layer: k 12, m 1, lists of 3, 38 MiB", 100, 32, 8, 12, 256, 1024, 1, True),
    ("k 4, m 4, lists of 4, 1 MiB", 2, 512, 512, 4, 128, 64, 4, False),
    ("enc1 at 8 frames: lists of 2, m 1, 256 MiB", 8, 16384, 4096, 8, 64, 256, 1, False),
    ("RCNN third layer: k 12, m 2, lists of 3, 96 MiB", 128, 128, 32, 12, 128, 512, 2, False),
    ("lists of 8, m 2, 12 MiB", 3, 512, 512, 8, 64, 128, 2, False)])
def test_route_taken_with_a_workspace_and_its_result(name, b, n, p, k, c0, c1, m, staged):
    """hf_xconv_depthwise_gather_grad through the C ABI with a workspace whose staging region holds a sentinel: the staged route
    overwrites the region, the direct route leaves every float of it; the route is the one xdw_fts_direct documents for the
    shape, and the table gradient equals, bit for bit, the no-workspace call and the materialised reference on both routes"""
    from heterofusionrcnn_amd import _lib, pointcnn as pc
    from heterofusionrcnn_amd._lib import check, ptr, stream_ptr
    from heterofusionrcnn_amd.grouping import concat_group, index_inverse
    L = _lib.lib()
    torch.manual_seed(b + n + p + k + c1 + m)
    dev, c = "cuda", c0 + c1
    x = torch.randn(b, p, k, k, device=dev)
    fd = torch.randn(b, p, k, c0, device=dev)
    fts = torch.randn(b, n, c1, device=dev, requires_grad=True)
    wd = torch.randn(k, c, m, device=dev)
    idx = torch.randint(0, n, (b, p, k), device=dev, dtype=torch.int32)
    off, ent = index_inverse(idx, n)
    go = torch.randn(b, p, c * m, device=dev)
    ref = torch.autograd.grad(pc.xconv_depthwise(x, concat_group(fd, fts, idx, (off, ent)), wd), fts, go)[0]
    nbytes = L.hf_xconv_depthwise_gather_grad_workspace(b, p, k, c0, c1, m)
    block = b * p * k * c1
    sentinel = 12345.0
    grads = []
    for with_ws in (True, False):
        ws = torch.full((nbytes // 4,), sentinel, dtype=torch.float32, device=dev)
        gx, gf, gt, gw = torch.empty_like(x), torch.empty_like(fd), torch.full_like(ref, 7.0), torch.empty_like(wd)
        check(L.hf_xconv_depthwise_gather_grad(b, n, p, k, c0, c1, m, ptr(x), ptr(fd), ptr(fts.detach()), ptr(idx), ptr(wd), ptr(go), ptr(off),
                                               ptr(ent), ptr(gx), ptr(gf), ptr(gt), ptr(gw), ptr(ws) if with_ws else None,
                                               nbytes if with_ws else 0, stream_ptr()), name)
        torch.cuda.synchronize()
        if with_ws:
            untouched = bool((ws[:block] == sentinel).all())
            assert untouched == (not staged), name
            assert not bool((ws[:block] == sentinel).any()) or not staged, name
        grads.append(gt)
        assert torch.equal(gt, ref), (name, with_ws)
    assert torch.equal(grads[0], grads[1]), name


def test_table_gradient_kernels_keep_their_state_in_registers(tmp_path):
    """compiled with the Makefile's flags: every xconv_dw_bwd_fts_kernel instantiation has no SGPR / VGPR spills, no scratch and
    at most 256 VGPRs"""
    asm = tmp_path / "xconv.s"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-ffp-contract=off",
                    "-std=c++17", "-I" + os.path.join(CSRC, "..", "..", "include"), "--cuda-device-only", "-S",
                    os.path.join(CSRC, "xconv.hip"), "-o", str(asm)], check=True, capture_output=True)
    text = asm.read_text()
    found = 0
    for blk in re.split(r"\n\s*- \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "xconv_dw_bwd_fts_kernel" not in name:
            continue
        found += 1
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
        assert field("sgpr_spill_count") == 0 and field("vgpr_spill_count") == 0, name
        assert field("private_segment_fixed_size") == 0, name
        assert field("vgpr_count") <= 256, name
    assert found == 8 * 2      # (K, M) pairs x whole-vector / single-float accesses
