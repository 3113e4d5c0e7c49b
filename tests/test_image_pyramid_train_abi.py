"""Kernel-level parity of the training kernels of csrc/conv_nhwc.hip through the C ABI (ctypes on _lib.lib(), no Python routing in
between) against the references and bounds of tests/image_pyramid_train_cases.py.  Inputs sit between NaN bands, outputs are
slices of sentinel-filled buffers pre-filled with NaN, workspaces sit between guard bands: a read or a write outside a tensor, or
an element never written, shows.  Every call is made twice and repeats its bits.  The exact family (every instantiation of the
weight-gradient kernel and of the stride-2 form) and the launch-regime cases are compared bit for bit, abi_harness.same."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_pyramid_cases as pc  # noqa: E402
import image_pyramid_train_cases as tc  # noqa: E402
from abi_harness import NAN, SENTINEL, WS_GUARD, Arena, In, Workspace, abi, call, dev64, same, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def inp(a, off=False):
    return None if a is None else In(DEV, a.copy(), off)


def p_of(i):
    return None if i is None else i.p


def run_wgrad(kind, name, off=False):
    """-> dwt (9, cout, cin) as the call wrote it; the arena and the workspace guards are checked"""
    _lib, L = abi()
    c = (tc.WGRAD_CASES if kind == "conv" else tc.UPWGRAD_CASES)[name]
    t = tc.wgrad_inputs(kind, name)
    query = L.hf_conv3x3_nhwc_wgrad_workspace if kind == "conv" else L.hf_upconv3x3s2_nhwc_wgrad_workspace
    nbytes = query(c["b"], c["h"], c["w"], c["cin"], c["cout"])
    a = Arena(DEV)
    dwt = a.out((9, c["cout"], c["cin"]))
    dwt.fill_(NAN)
    ws = Workspace(DEV, nbytes)
    ws.buf[WS_GUARD:WS_GUARD + nbytes] = 0xff                              # NaN bit patterns: a partial tile read before it is written shows
    x, dz, sub = inp(t["x"], off), inp(t["dz"]), inp(t["in_sub"])
    wsp = ws.p if nbytes else None
    if kind == "conv":
        call(L.hf_conv3x3_nhwc_wgrad(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, p_of(sub), dz.p, ctypes.c_void_p(dwt.data_ptr()), wsp,
                                     nbytes, _lib.stream_ptr()), "hf_conv3x3_nhwc_wgrad")
    else:
        call(L.hf_upconv3x3s2_nhwc_wgrad(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, dz.p, ctypes.c_void_p(dwt.data_ptr()), wsp, nbytes,
                                         _lib.stream_ptr()), "hf_upconv3x3s2_nhwc_wgrad")
    a.check()
    ws.check(name)
    return dwt.clone(), nbytes


def check_wgrad(kind, name):
    c = (tc.WGRAD_CASES if kind == "conv" else tc.UPWGRAD_CASES)[name]
    r = tc.wgrad_reference(kind, name)
    got, nbytes = run_wgrad(kind, name)
    assert (nbytes == 0) == (c["b"] * c["h"] * c["w"] <= 256), "a single chunk needs no workspace, several need one"
    assert torch.equal(got, run_wgrad(kind, name)[0]), "two calls differ"
    within(got, dev64(DEV, r["dwt"].numpy()), dev64(DEV, r["bound"].numpy()),
           "hf_conv3x3_nhwc_wgrad" if kind == "conv" else "hf_upconv3x3s2_nhwc_wgrad", "rows %d" % (c["b"] * c["h"] * c["w"]))
    if (c["h"], c["w"]) == (1, 1):
        # one pixel: the convolution's centre tap alone sees it; the up-convolution's pixel feeds outputs (ky - 1, kx - 1), ky, kx >= 1
        live = (4,) if kind == "conv" else (4, 5, 7, 8)
        assert all(bool((got[t] == 0).all()) for t in range(9) if t not in live), "a tap that pairs the pixel with padding is not zero"


@pytest.mark.parametrize("name", list(tc.WGRAD_CASES))
def test_conv3x3_wgrad(name):
    check_wgrad("conv", name)


@pytest.mark.parametrize("name", list(tc.UPWGRAD_CASES))
def test_upconv3x3s2_wgrad(name):
    check_wgrad("up", name)


def test_wgrad_off_the_16_byte_boundary_takes_the_scalar_path():
    """x one float past a 16-byte boundary: the scalar staging path of the X operand, the same sums in the same order, the same bits"""
    name = "b1h12w22_ci36_co40"
    aligned, moved = run_wgrad("conv", name)[0], run_wgrad("conv", name, off=True)[0]
    assert not torch.isnan(aligned).any() and torch.equal(aligned, moved)


def run_s2(name):
    _lib, L = abi()
    c, t = tc.S2_CASES[name], tc.s2_inputs(name)
    stride, col = pc.slice_of(c)
    rows = c["b"] * c["h"] * c["w"]
    a = Arena(DEV)
    wide = a.out((rows, stride))
    wide[:, col:col + c["cout"]] = NAN
    x, wt, scale, shift = (inp(t[k]) for k in ("x", "wt", "scale", "shift"))
    call(L.hf_conv3x3s2_nhwc(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, wt.p, p_of(scale), p_of(shift), int(c["relu"]),
                             ctypes.c_void_p(wide.data_ptr()), stride, col, _lib.stream_ptr()), "hf_conv3x3s2_nhwc")
    a.check()
    beside = torch.cat([wide[:, :col], wide[:, col + c["cout"]:]], dim=1)
    assert bool((beside == SENTINEL).all()), "a column outside [y_col, y_col + cout) was written"
    return wide[:, col:col + c["cout"]].clone()


@pytest.mark.parametrize("name", list(tc.S2_CASES))
def test_conv3x3s2(name):
    c, r = tc.S2_CASES[name], tc.s2_reference(name)
    got = run_s2(name)
    assert torch.equal(got, run_s2(name)), "two calls differ"
    within(got, dev64(DEV, r["y"].numpy()), dev64(DEV, r["bound"].numpy()), "hf_conv3x3s2_nhwc", "cin %d" % c["cin"])
    if c["relu"]:
        assert bool((got >= 0).all())


def run_dgrad(name):
    """hf_conv3x3_nhwc on dz with the flipped, transposed weights, into a slice: cin and cout change places"""
    _lib, L = abi()
    c, t = pc.CONV_CASES[name], tc.dgrad_inputs(name)
    rows, stride, col = c["b"] * c["h"] * c["w"], 2 * c["cin"] + 4, c["cin"]
    a = Arena(DEV)
    wide = a.out((rows, stride))
    wide[:, col:col + c["cin"]] = NAN
    dz, wd = inp(t["dz"]), inp(t["wd"])
    call(L.hf_conv3x3_nhwc(c["b"], c["h"], c["w"], c["cout"], c["cin"], dz.p, None, wd.p, None, None, 0, ctypes.c_void_p(wide.data_ptr()),
                           stride, col, _lib.stream_ptr()), "hf_conv3x3_nhwc")
    a.check()
    beside = torch.cat([wide[:, :col], wide[:, col + c["cin"]:]], dim=1)
    assert bool((beside == SENTINEL).all())
    return wide[:, col:col + c["cin"]].clone()


@pytest.mark.parametrize("name", list(tc.DGRAD_CASES))
def test_dgrad_through_the_forward_kernel(name):
    r = tc.dgrad_reference(name)
    got = run_dgrad(name)
    assert torch.equal(got, run_dgrad(name)), "two calls differ"
    within(got, dev64(DEV, r["dx"].numpy()), dev64(DEV, r["bound"].numpy()), "hf_conv3x3_nhwc as dgrad", "cout %d" % pc.CONV_CASES[name]["cout"])


def run_pool_bwd(name, accumulate, sliced, c=None, t=None):
    """-> the (rows, c) slice of dx after the call, on the host; c, t: a case and inputs outside POOL_BWD_CASES"""
    _lib, L = abi()
    c, t = (tc.POOL_BWD_CASES[name], tc.pool_bwd_inputs(name)) if c is None else (c, t)
    ch = c["c"]
    stride, col = (2 * ch + 4, ch) if sliced else (ch, 0)
    rows = t["x"].reshape(-1, ch)
    xwide = np.full((rows.shape[0], stride), np.nan, dtype=np.float32)     # a read beside the slice is a NaN, and a NaN wins
    xwide[:, col:col + ch] = rows
    a = Arena(DEV)
    wide = a.out((rows.shape[0], stride))
    wide[:, col:col + ch] = torch.from_numpy(t["base"].reshape(-1, ch).copy()).to(DEV) if accumulate else NAN
    x, g = In(DEV, xwide), inp(t["g"])
    call(L.hf_maxpool2x2_nhwc_bwd(c["b"], c["h"], c["w"], ch, x.p, stride, col, g.p, ctypes.c_void_p(wide.data_ptr()), stride, col,
                                  accumulate, _lib.stream_ptr()), "hf_maxpool2x2_nhwc_bwd")
    a.check()
    beside = torch.cat([wide[:, :col], wide[:, col + ch:]], dim=1)
    assert bool((beside == SENTINEL).all()), "a column outside [dx_col, dx_col + c) was written"
    return wide[:, col:col + ch].cpu().numpy().copy()


@pytest.mark.parametrize("name", list(tc.POOL_BWD_CASES))
def test_maxpool2x2_bwd_is_torch_bit_for_bit(name):
    c, t, e = tc.POOL_BWD_CASES[name], tc.pool_bwd_inputs(name), tc.pool_bwd_expected(name)
    for sliced in (True, False):
        for accumulate in (0, 1):
            got = run_pool_bwd(name, accumulate, sliced)
            again = run_pool_bwd(name, accumulate, sliced)
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two calls differ"
            got = got.reshape(t["x"].shape)
            if accumulate:
                want = e["sum"]            # base + torch's gradient, one fp32 add; a last odd row or column adds zero: the base's bits
                assert np.array_equal(got[:, c["h"] // 2 * 2:].view(np.uint32), t["base"][:, c["h"] // 2 * 2:].view(np.uint32))
                assert np.array_equal(got[:, :, c["w"] // 2 * 2:].view(np.uint32), t["base"][:, :, c["w"] // 2 * 2:].view(np.uint32))
            else:
                want = e["grad"]
                assert not got[:, c["h"] // 2 * 2:].any() and not got[:, :, c["w"] // 2 * 2:].any(), "the dropped odd row or column is not zero"
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, sliced, accumulate)


@pytest.mark.parametrize("name", list(pc.REGIME_POOL_BWD_CASES))
def test_maxpool2x2_bwd_grid_stride_regime_is_torch_bit_for_bit(name):
    """more cells than the capped grid has lanes, the cells of the last odd row and column among them: every lane takes a second
    item; from a slice and dense, writing and accumulating"""
    c, t = pc.REGIME_POOL_BWD_CASES[name], pc.regime_pool_inputs(name, backward=True)
    assert pc.pool_strides(c, True, backward=True) and pc.pool_strides(c, False, backward=True) and c["h"] % 2 and c["w"] % 2
    x = torch.from_numpy(t["x"]).permute(0, 3, 1, 2).contiguous().requires_grad_()
    torch.nn.functional.max_pool2d(x, 2).backward(torch.from_numpy(t["g"]).permute(0, 3, 1, 2).contiguous())
    grad = x.grad.permute(0, 2, 3, 1).contiguous().numpy()
    assert not grad[:, -1].any() and not grad[:, :, -1].any()
    for sliced in (True, False):
        for accumulate in (0, 1):
            got = run_pool_bwd(name, accumulate, sliced, c, t)
            again = run_pool_bwd(name, accumulate, sliced, c, t)
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two calls differ"
            want = t["base"] + grad if accumulate else grad          # one fp32 add; the dropped row and column add zero: the base's bits
            assert np.array_equal(got.reshape(want.shape).view(np.uint32), want.view(np.uint32)), (name, sliced, accumulate)


# ------------------------------------------------------------------------------------------------ the exact family
def run_exact_s2(c, t):
    _lib, L = abi(unset=("HF_GEMM_ROUNDS",))
    stride, col = pc.slice_of(c)
    a = Arena(DEV)
    wide = a.out((pc.conv_rows(c), stride))
    wide[:, col:col + c["cout"]] = NAN
    x, wt = In(DEV, t["x"], c["off"] == "x"), In(DEV, t["wt"], c["off"] == "wt")
    scale, shift = (None if t[k] is None else In(DEV, t[k]) for k in ("scale", "shift"))
    call(L.hf_conv3x3s2_nhwc(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, wt.p, p_of(scale), p_of(shift), int(c["relu"]),
                             ctypes.c_void_p(wide.data_ptr()), stride, col, _lib.stream_ptr()), "hf_conv3x3s2_nhwc")
    a.check()
    if col:
        assert bool((wide[:, :col] == SENTINEL).all()) and bool((wide[:, col + c["cout"]:] == SENTINEL).all()), \
            "a column outside [y_col, y_col + cout) was written"
    return wide[:, col:col + c["cout"]].clone()


@pytest.mark.parametrize("name", list(tc.EXACT_S2_CASES))
def test_conv3x3s2_exact(name):
    c, t, y, smax = pc.exact_conv_case("s2", name)
    assert pc.exact_condition(smax)
    got = run_exact_s2(c, t)
    assert torch.equal(got, run_exact_s2(c, t)), "two calls differ"
    same(got, y.to(DEV), "%s s2 %s" % (pc.conv_instantiation(c, c["off"]), name))


@pytest.mark.parametrize("name", list(tc.REGIME_S2_CASES))
def test_conv3x3s2_persistent_grid_regime_exact(name):
    """exact inputs at a production grid size; the fp64 tap sums are formed on the device by torch, not by this library"""
    c = tc.REGIME_S2_CASES[name]
    fewest, most = pc.conv_tiles(c)
    assert fewest >= 2 and most >= 3 and pc.conv_rows(c) % pc.FWD_ROWS
    t = pc.exact_conv_inputs(name, c)
    got = run_exact_s2(c, t)
    assert torch.equal(got, run_exact_s2(c, t)), "two calls differ"
    y, smax = pc.exact_conv_reference(c, t, device=DEV)
    assert pc.exact_condition(smax)
    same(got, y, "%s s2 regime %s" % (pc.conv_instantiation(c), name))


def run_exact_wgrad(c, t):
    _lib, L = abi()
    plan = tc.conv_wgrad_plan(c)
    query = L.hf_upconv3x3s2_nhwc_wgrad_workspace if c["up"] else L.hf_conv3x3_nhwc_wgrad_workspace
    nbytes = query(c["b"], c["h"], c["w"], c["cin"], c["cout"])
    assert nbytes == plan["workspace"], "the workspace is not the restated plan's: %d chunks" % plan["chunks"]
    a = Arena(DEV)
    dwt = a.out((9, c["cout"], c["cin"]))
    dwt.fill_(NAN)
    ws = Workspace(DEV, nbytes)
    ws.buf[WS_GUARD:WS_GUARD + nbytes] = 0xff                              # NaN bit patterns: a partial tile read before it is written shows
    x, dz = In(DEV, t["x"], c["off"] == "x"), In(DEV, t["dz"], c["off"] == "dz")
    sub = None if t["in_sub"] is None else In(DEV, t["in_sub"])
    wsp = ws.p if nbytes else None
    if c["up"]:
        call(L.hf_upconv3x3s2_nhwc_wgrad(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, dz.p, ctypes.c_void_p(dwt.data_ptr()), wsp, nbytes,
                                         _lib.stream_ptr()), "hf_upconv3x3s2_nhwc_wgrad")
    else:
        call(L.hf_conv3x3_nhwc_wgrad(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, p_of(sub), dz.p, ctypes.c_void_p(dwt.data_ptr()), wsp,
                                     nbytes, _lib.stream_ptr()), "hf_conv3x3_nhwc_wgrad")
    a.check()
    ws.check("exact wgrad")
    return dwt.clone()


def check_exact_wgrad(up, name):
    c, t, dwt, smax = tc.exact_wgrad_case(up, name)
    assert smax < 2 ** 24
    got = run_exact_wgrad(c, t)
    assert torch.equal(got, run_exact_wgrad(c, t)), "two calls differ"
    same(got, dwt.to(DEV), "%s %s" % (tc.wgrad_instantiation(c, c["off"]), name))
    if (c["h"], c["w"]) == (1, 1):
        live = (4, 5, 7, 8) if up else (4,)
        assert all(bool((got[t] == 0).all()) for t in range(9) if t not in live), "a tap that pairs the pixel with padding is not zero"


@pytest.mark.parametrize("name", list(tc.EXACT_WGRAD_CASES))
def test_conv3x3_wgrad_exact(name):
    check_exact_wgrad(False, name)


@pytest.mark.parametrize("name", list(tc.EXACT_UPWGRAD_CASES))
def test_upconv3x3s2_wgrad_exact(name):
    check_exact_wgrad(True, name)


def test_bad_arguments_return_einval_and_launch_nothing():
    _lib, L = abi()
    a = Arena(DEV)
    buf = a.out((4096,))
    wrong = {k: v for k, v in tc.einval_calls(L, ctypes.c_void_p(buf.data_ptr())).items() if v != _lib.HF_EINVAL}
    assert not wrong, wrong
    a.untouched()
