"""tests/xconv_cases.py checked on any machine: the fp64 references against torch fp64 autograd, the exact family's 2^24 limit, every
case's regime from the restated geometry, the sensitivity of the rounding bounds, and the argument checks of the entry points of
csrc/xconv.hip that return before any launch (fake non-null pointers, never dereferenced)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xconv_cases as xc  # noqa: E402

CASES = xc.all_cases()


def test_case_ids_are_unique_and_counted():
    ids = [xc.case_id(c) for c in CASES]
    assert len(ids) == len(set(ids))
    assert len(ids) == 512, "a case was added or removed: update this number when you add a case"


def test_every_dispatch_pair_is_known():
    for c in CASES:
        if c["kind"] in ("fwd", "bwd"):
            assert (c["k"], c["m"]) in xc.XDW_DISPATCH and c["c0"] % 64 == 0
        elif c["kind"] in ("dw", "dw_grad"):
            assert (c["k"], c["m"]) in xc.DW_DISPATCH
        else:
            assert c["k"] in xc.APPLY_K


def test_exact_family_stays_below_two_to_the_24():
    for c in CASES:
        if c["family"] == "exact":
            assert xc.exact_worst(c) < xc.EXACT_LIMIT, xc.case_id(c)
    t = xc.make_inputs(next(c for c in CASES if c["family"] == "exact" and c["kind"] == "bwd"))
    for name in ("x", "fd", "fts", "wd", "go"):
        assert np.abs(t[name]).max() <= xc.EXACT_A and np.array_equal(t[name], np.round(t[name]))


def _fwd_trips(c):
    """(rows per block, trips of wave 0 over its rows) of the forward kernel"""
    _, _, rpb = xc.xdw_pair_grid(xc.rows_of(c), c["c0"] + c["c1"])
    return rpb, xc.cdiv(rpb, xc.WAVES * xc.XC_ROWS)


def _regime(c):
    """asserts, from the restated geometry, that the case is in the regime it is named for"""
    r, rows = c["regime"], xc.rows_of(c)
    k, m = c["k"], c.get("m", 0)
    if c["kind"] == "fwd":
        ch = c["c0"] + c["c1"]
        gx, gy, rpb = xc.xdw_pair_grid(rows, ch)
        v2 = xc.xdw_v2(ch, xc.aligned(c, "f", "fts", "out"))
        assert xc.offsets_fit(rows, k, ch, c["b"] * c["n"])
        if r == "block4":
            assert rpb == 4 and rows % 4 != 0 and gx > 1 and ch % 128 != 0 and v2 and c["p"] == 7
        elif r == "c_odd":
            assert ch % 2 == 1 and not v2 and c["p"] == 3 and rpb == 4 and rows % 4 != 0
        elif r in ("trips", "cloud3_trips"):
            assert rpb > 8 and rpb % 8 != 0 and _fwd_trips(c)[1] == 2 and gx > 1 and c["p"] in (3, 7) and rpb % c["p"] != 0
        elif r == "cloud1":
            assert c["p"] == 1 and gx > 1
        elif r == "v2_off_align":
            assert ch % 2 == 0 and not v2 and len(c["off"]) == 1
        elif r == "straddle64":
            assert c["c0"] == 64 and ch >= 128
        elif r == "straddle192":
            assert c["c0"] == 192 and ch >= 256
        elif r == "c1_one":
            assert c["c1"] == 1
        else:
            raise AssertionError(r)
    elif c["kind"] == "bwd":
        ch = c["c0"] + c["c1"]
        gx, gy, rpb = xc.xdw_bwd_grid(rows, ch) if rows else (0, 0, 0)
        src = c["b"] * c["n"]
        vec = xc.fts_vec(c["c1"], m, xc.aligned(c, "go", "gfts"))
        if r in ("rows_le_32", "subset", "n_src_small", "rows_32", "single_block"):
            assert rows <= 32 and rpb == min(rows, 4) and gx == xc.cdiv(rows, 4) and ch % 64 != 0
            assert (r != "rows_32" or rows == 32) and (r != "single_block" or gx == 1)
            if r == "rows_le_32":
                assert vec and (not c["gather"] or xc.fts_grid(src, c["c1"], m)[2] == 4)
            if r == "n_src_small":
                assert c["n"] in (1, 2, 3)
        elif r == "vec_off_c1":
            assert not vec and c["c1"] % xc.fts_cpl(m) != 0
        elif r == "floor32":
            assert 32 < rows < 64 and rpb == 32 and gx == 2 and xc.xdw_grid(rows, ch, 4)[2] < 32
        elif r in ("go_off", "gfts_off"):
            assert not vec and c["c1"] % xc.fts_cpl(m) == 0
        elif r == "ragged_blocks":
            assert rpb > 32 and rows % rpb != 0 and gx > 16
        elif r == "rows_gt_8192":
            assert rows > xc.MAX_BLOCKS * xc.WAVES and xc.grid_for(rows, xc.WAVES) == xc.MAX_BLOCKS and ch <= 128
        elif r == "no_rows":
            assert rows == 0 and c["b"] > 0 and c["n"] > 0 and not xc.instantiations(c)
        elif r == "table_trips":
            assert xc.fts_grid(src, c["c1"], m)[2] > 8 and xc.route(c) == "direct" and vec
        elif r.startswith("staged"):
            assert xc.route(c) == "staged" and c["p"] * k < 8 * c["n"] and 8 * xc.MIB < xc.staged_bytes(rows, k, c["c1"]) < 80 * xc.MIB
            if r == "staged":
                assert xc.staged_bytes(rows, k, c["c1"]) < 9 * xc.MIB
        elif r == "direct_8MiB":
            assert xc.route(c) == "direct" and c["p"] * k < 8 * c["n"] and xc.staged_bytes(rows, k, c["c1"]) == 8 * xc.MIB
        elif r == "direct_lists_of_8":
            assert xc.route(c) == "direct" and c["p"] * k == 8 * c["n"] and xc.staged_bytes(rows, k, c["c1"]) > 8 * xc.MIB
        elif r == "direct_80MiB":
            assert xc.route(c) == "direct" and c["p"] * k < 8 * c["n"] and xc.staged_bytes(rows, k, c["c1"]) == 80 * xc.MIB and m <= 2
        else:
            raise AssertionError(r)
    elif c["kind"] in ("apply", "apply_grad"):
        if r == "rows_gt_8192":
            assert rows > xc.MAX_BLOCKS * xc.WAVES
        else:
            assert r == "small" and c["c"] % 64 != 0
    else:
        ch = c["c"]
        narrow = xc.is_narrow(ch, k, m)
        if r in ("narrow", "narrow_small"):
            assert narrow and (r == "narrow_small" or 256 % ch != 0)
        elif r == "narrow_loop":
            assert narrow and 256 % ch != 0 and rows * ch > xc.narrow_grid(rows, ch) * xc.THREADS
        elif r == "wide":
            assert not narrow
        elif r == "wide_loop":
            assert not narrow and rows * ch > xc.MAX_BLOCKS * xc.THREADS
        elif r == "want_x":
            assert c["want"] == ("x",)
        elif r.startswith("dw_"):
            assert r == "dw_" + xc.dw_reduction(ch) and rows in xc.DW_SWEEP_ROWS
            if rows == 203:
                _, rpc, nchunks = xc.dw_chunks(rows, ch)
                assert nchunks > 1 and rows % rpc != 0
        else:
            raise AssertionError(r)


@pytest.mark.parametrize("c", CASES, ids=xc.case_id)
def test_case_is_in_its_regime(c):
    _regime(c)


def test_the_case_table_holds_what_it_must():
    ids = {xc.case_id(c) for c in CASES}
    exact = [c for c in CASES if c["family"] == "exact"]
    for k, m in xc.XDW_DISPATCH:
        for g in (True, False):
            for regime in ("block4", "trips", "c_odd"):
                assert any(c["kind"] == "fwd" and c["regime"] == regime and (c["k"], c["m"], c["gather"]) == (k, m, g) for c in exact)
            assert any(c["kind"] == "bwd" and c["regime"] == "rows_le_32" and (c["k"], c["m"], c["gather"]) == (k, m, g) for c in exact)
        for regime in ("vec_off_c1", "floor32"):
            assert any(c["kind"] == "bwd" and c["regime"] == regime and (c["k"], c["m"]) == (k, m) for c in exact)
    for group in xc.DW_SWEEP_C:
        for ch in group:
            for rows in xc.DW_SWEEP_ROWS:
                for ws in (True, False):
                    assert any(c["kind"] == "dw_grad" and (c["rows"], c["c"], c["ws"]) == (rows, ch, ws) and c["regime"].startswith("dw_") for c in exact)
    assert {xc.dw_reduction(ch) for ch in xc.DW_SWEEP_C[0]} == {"shuffle"} and {xc.dw_reduction(ch) for ch in xc.DW_SWEEP_C[1]} == {"lds"}
    assert {xc.dw_reduction(ch) for ch in xc.DW_SWEEP_C[2]} == {"one_slot"}
    # the neighbour tables: the lists around kFtsEntries, one row named by every slot, the last row unnamed; the forward's table edges
    c = next(c for c in exact if c["kind"] == "bwd" and c["regime"] == "rows_le_32" and c["gather"] and c["k"] == 8)
    idx = xc.make_inputs(c)["idx"]
    lens = xc.list_lengths(idx, c["n"])
    assert {0, 1, 4, 5, 8, 9} <= set(lens[1].tolist()) and lens[0].max() == c["p"] * c["k"] and lens[-1][-1] == 0
    c = next(c for c in exact if c["kind"] == "fwd" and c["regime"] == "block4" and c["gather"])
    idx = xc.make_inputs(c)["idx"]
    for cloud in (0, -1):
        assert {0, c["n"] - 1} <= set(idx[cloud, 0].tolist()) and {0, c["n"] - 1} <= set(idx[cloud, -1].tolist())
    assert len(ids) == len(CASES)


def test_geometry_restated_from_the_launchers():
    assert xc.grid_for(0, 4) == 1 and xc.grid_for(8192, 4) == 2048 and xc.grid_for(10 ** 7, 4) == 2048
    assert xc.narrow_grid(65, 3) % 3 == 0 and xc.narrow_grid(10 ** 6, 3) == 2049 and xc.narrow_grid(10 ** 6, 8) == 2048
    assert xc.dw_chunks(1, 8) == (1, 1, 1) and xc.dw_chunks(131072, 8) == (1, 256, 512) and xc.dw_chunks(203, 640) == (3, 51, 4)
    assert xc.xdw_pair_grid(21, 134) == (6, 2, 4) and xc.xdw_pair_grid(1701, 1280) == (189, 10, 9)
    assert xc.xdw_bwd_grid(33, 100) == (2, 2, 32) and xc.xdw_bwd_grid(32, 100) == (8, 2, 4) and xc.xdw_bwd_grid(1701, 1280) == (52, 20, 33)
    assert xc.fts_grid(1100, 2048, 2) == (123, 16, 9) and xc.fts_grid(39, 36, 1) == (10, 1, 4)
    assert xc.gather_grad_workspace(3, 7, 8, 64, 36, 2) == ((4 * 21 * 8 * 36 + 255) & ~255) + 4 * 6 * 8 * 100 * 2
    assert xc.gather_grad_workspace(0, 7, 8, 64, 36, 2) == 0 and xc.dw_grad_workspace(203, 8, 640, 2) == 4 * 4 * 8 * 640 * 2
    assert not xc.offsets_fit(1 << 20, 8, 512, 0) and xc.offsets_fit((1 << 20) - 1, 8, 512, 0)


# ------------------------------------------------------------------------------------------------- references against autograd
def _torch_fused(c, t):
    x, fd, fts, wd = (torch.tensor(t[n], dtype=torch.float64, requires_grad=True) for n in ("x", "fd", "fts", "wd"))
    b, p, n, k = c["b"], c["p"], c["n"], c["k"]
    rows = (torch.arange(b)[:, None, None] * n + torch.from_numpy(t["idx"]).long()).reshape(b * p, k)
    f = torch.cat([fd, fts[rows]], dim=2)
    out = torch.einsum("rkc,kcm->rcm", torch.matmul(x, f), wd).reshape(b * p, -1)
    grads = torch.autograd.grad(out, (x, fd, wd, fts), torch.tensor(t["go"], dtype=torch.float64))
    return out.detach().numpy(), dict(zip(("x", "f", "wd", "fts"), (g.numpy() for g in grads)))


@pytest.mark.parametrize("k,m,b,p,n,c0,c1", [(8, 2, 3, 7, 13, 64, 36), (4, 4, 2, 5, 3, 64, 7), (12, 1, 4, 3, 2, 128, 1)])
def test_fused_references_equal_fp64_autograd(k, m, b, p, n, c0, c1):
    c = xc._fused("bwd", "round", "rows_le_32", k, m, True, b, p, n, c0, c1)
    t = xc.make_inputs(c)
    out, grads = _torch_fused(c, t)
    np.testing.assert_allclose(xc.ref_fused_fwd(c, t), out, rtol=1e-12, atol=1e-12)
    ref = xc.ref_fused_bwd(c, t, xc.ALL4)
    for name in xc.ALL4:
        np.testing.assert_allclose(ref[name], grads[name], rtol=1e-12, atol=1e-12, err_msg=name)
    only = xc.ref_fused_bwd(c, t, ("fts",))
    np.testing.assert_allclose(only["fts"], grads["fts"], rtol=1e-12, atol=1e-12)
    dense = xc.ref_fused_bwd(dict(c, gather=False), t, ("f",))["f"]
    np.testing.assert_allclose(dense[:, :, :c0], grads["f"], rtol=1e-12, atol=1e-12)
    # the magnitude sums dominate the values
    mag = xc.ref_fused_bwd(c, t, xc.ALL4, mag=True)
    assert all((np.abs(ref[name]) <= mag[name] * (1 + 1e-12)).all() for name in xc.ALL4)


def test_two_kernel_references_equal_fp64_autograd():
    c = xc._two("apply_grad", "round", "small", 8, 0, 11, 37, want=("x", "f"))
    t = xc.make_inputs(c)
    x, f = (torch.tensor(t[n], dtype=torch.float64, requires_grad=True) for n in ("x", "f"))
    out = torch.matmul(x, f)
    gx, gf = torch.autograd.grad(out, (x, f), torch.tensor(t["go"], dtype=torch.float64))
    np.testing.assert_allclose(xc.ref_apply(t), out.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xc.ref_apply_grad(t)["x"], gx.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xc.ref_apply_grad(t)["f"], gf.numpy(), rtol=1e-12, atol=1e-12)
    c = xc._two("dw_grad", "round", "wide", 8, 3, 19, 70, want=("x", "w"), ws=False)
    t = xc.make_inputs(c)
    x, w = (torch.tensor(t[n], dtype=torch.float64, requires_grad=True) for n in ("x", "w"))
    y = torch.einsum("rwc,wcm->rcm", x, w).reshape(19, -1)
    gx, gw = torch.autograd.grad(y, (x, w), torch.tensor(t["go"], dtype=torch.float64))
    np.testing.assert_allclose(xc.ref_dw(t), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xc.ref_dw_grad(t)["x"], gx.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xc.ref_dw_grad(t)["w"], gw.numpy(), rtol=1e-12, atol=1e-12)


def test_index_inverse_lists_positions_in_ascending_order():
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 5, (2, 4, 8)).astype(np.int32)
    off, ent = xc.index_inverse(idx, 5)
    for b in range(2):
        flat = idx[b].reshape(-1)
        for s in range(5):
            assert ent[b, off[b, s]:off[b, s + 1]].tolist() == [i for i in range(32) if flat[i] == s]


# ------------------------------------------------------------------------------------------------- sensitivity of the bounds
def _f32_sum(terms, order):
    s = np.float32(0)
    for i in order:
        s = np.float32(s + terms[i])
    return s


def test_rounding_bounds_admit_another_order_and_reject_a_dropped_term():
    """grad_wd and grad_fts of a rounding case on the CPU: the same sums in fp32, with every product rounded and the terms added in a
    shuffled order, stay inside n u M; the fp64 reference with one row (grad_wd) or one neighbour slot (grad_fts) dropped falls outside
    it for the elements that lose the term"""
    c = next(c for c in CASES if c["kind"] == "bwd" and c["family"] == "round" and c["regime"] == "rows_le_32" and c["gather"] and (c["k"], c["m"]) == (8, 2))
    t = xc.make_inputs(c)
    ref, mag, n = xc.ref_fused_bwd(c, t, xc.ALL4), xc.ref_fused_bwd(c, t, xc.ALL4, mag=True), xc.roundings(c, t)
    rng = np.random.default_rng(0)
    rows, k, m = xc.rows_of(c), c["k"], c["m"]
    f32 = xc.concat_f(c, t).astype(np.float32)
    fx = np.zeros((rows, k, f32.shape[2]), np.float32)
    for j in range(k):
        fx = (fx + t["x"][:, :, j, None] * f32[:, None, j, :]).astype(np.float32)
    terms = (fx[:, :, :, None] * t["go"].reshape(rows, 1, -1, m)).astype(np.float32)              # (rows, k, c, m)
    shuffled = np.zeros(terms.shape[1:], np.float32)
    for r in rng.permutation(rows):
        shuffled = (shuffled + terms[r]).astype(np.float32)
    assert (np.abs(shuffled - ref["wd"]) <= xc.bound(n["wd"], mag["wd"])).all()
    t2 = dict(t, go=t["go"].copy())
    t2["go"][5] = 0                                                                                # row 5 dropped from the sum
    dropped = xc.ref_fused_bwd(c, t2, ("wd",))["wd"]
    lost = np.abs(dropped - ref["wd"])
    assert (lost > xc.bound(n["wd"], mag["wd"]))[lost > 1e-3 * mag["wd"]].all() and (lost > 1e-3 * mag["wd"]).mean() > 0.5
    # one neighbour slot of the table gradient
    r, j = 9, 3
    s = c["n"] * (r // c["p"]) + int(t["idx"].reshape(rows, k)[r, j])
    t3 = dict(t, x=t["x"].copy())
    t3["x"][r, :, j] = 0                                                                           # dF[r][j][:] = 0
    dropped = xc.ref_fused_bwd(c, t3, ("fts",))["fts"]
    b = xc.bound(n["fts"], mag["fts"])
    lost = np.abs(dropped - ref["fts"])
    assert (lost[s] > b[s]).mean() > 0.9 and (np.delete(lost, s, axis=0) == 0).all()


def test_forward_bound_admits_fp32_and_rejects_a_dropped_neighbour():
    c = next(c for c in CASES if c["kind"] == "fwd" and c["family"] == "round" and c["regime"] == "block4" and c["gather"] and (c["k"], c["m"]) == (8, 2))
    t = xc.make_inputs(c)
    ref, mag, n = xc.ref_fused_fwd(c, t), xc.ref_fused_fwd(c, t, mag=True), xc.roundings(c)["out"]
    f32 = xc.concat_f(c, t).astype(np.float32)
    rows, k, m = xc.rows_of(c), c["k"], c["m"]
    out = np.zeros((rows, f32.shape[2], m), np.float32)
    for kk in reversed(range(k)):                                                                  # the other order
        fx = np.zeros((rows, f32.shape[2]), np.float32)
        for j in reversed(range(k)):
            fx = (fx + t["x"][:, kk, j, None] * f32[:, j, :]).astype(np.float32)
        out = (out + fx[:, :, None] * t["wd"][kk][None]).astype(np.float32)
    assert (np.abs(out.reshape(rows, -1) - ref) <= xc.bound(n, mag)).all()
    t2 = dict(t, x=t["x"].copy())
    t2["x"][:, :, 2] = 0                                                                           # neighbour slot 2 dropped
    lost = np.abs(xc.ref_fused_fwd(c, t2) - ref)
    assert (lost > xc.bound(n, mag)).mean() > 0.99


# ------------------------------------------------------------------------------------------------- argument checks before any launch
def test_entry_points_reject_bad_arguments_without_a_gpu():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(256)      # never dereferenced: every call below fails its argument check first
    EINVAL, EWS = _lib.HF_EINVAL, _lib.HF_EWORKSPACE
    big = ctypes.c_size_t(1 << 40)

    def gather(b=2, n=5, p=7, k=8, c0=64, c1=36, m=1, out=fake):
        return L.hf_xconv_depthwise_gather(b, n, p, k, c0, c1, m, fake, fake, fake, fake, fake, out, None)

    def gather_grad(b=2, n=5, p=7, k=8, c0=64, c1=36, m=1, off=fake, ent=fake, gx=fake, gfts=fake, ws=None, nbytes=0):
        return L.hf_xconv_depthwise_gather_grad(b, n, p, k, c0, c1, m, fake, fake, fake, fake, fake, fake, off, ent, gx, None, gfts, None, ws, nbytes, None)

    bad = {
        "fused: unsupported (k, m)": L.hf_xconv_depthwise(10, 8, 64, 8, fake, fake, fake, fake, None),
        "fused: k = 5": L.hf_xconv_depthwise(10, 5, 64, 1, fake, fake, fake, fake, None),
        "fused: (12, 4)": L.hf_xconv_depthwise(10, 12, 64, 4, fake, fake, fake, fake, None),
        "fused: rows k c = 2^32": L.hf_xconv_depthwise(1 << 20, 8, 512, 1, fake, fake, fake, fake, None),
        "fused: c = 0": L.hf_xconv_depthwise(10, 8, 0, 1, fake, fake, fake, fake, None),
        "fused: no output": L.hf_xconv_depthwise(10, 8, 64, 1, fake, fake, fake, None, None),
        "gather: c0 % 64": gather(c0=32), "gather: c0 = 0": gather(c0=0), "gather: c1 = 0": gather(c1=0), "gather: n_src = 0": gather(n=0),
        "gather: (8, 8)": gather(m=8), "gather: b rows_per_cloud > 2^31 - 1": gather(b=1 << 16, p=1 << 15),
        "gather: rows k c = 2^32": gather(b=1 << 10, p=1 << 10, c0=448, c1=64), "gather: table of 2^32 elements": gather(b=1 << 12, n=1 << 11, p=1, c0=448, c1=64),
        "gather: no output": gather(out=None),
        "gather grad: c0 % 64": gather_grad(c0=96), "gather grad: b rows_per_cloud > 2^31 - 1": gather_grad(b=1 << 16, p=1 << 15),
        "gather grad: grad_fts without offsets": gather_grad(off=None), "gather grad: grad_fts without entries": gather_grad(ent=None),
        "gather grad: nothing asked for": gather_grad(gx=None, gfts=None),
        "apply: k = 12": L.hf_xconv_apply(10, 12, 64, fake, fake, fake, None),
        "apply grad: nothing asked for": L.hf_xconv_apply_grad(10, 8, 64, fake, fake, fake, None, None, None),
        "depthwise: (8, 5)": L.hf_depthwise_k(10, 8, 64, 5, fake, fake, fake, None),
        "depthwise: (12, 1)": L.hf_depthwise_k(10, 12, 100, 1, fake, fake, fake, None),
        "depthwise grad: nothing asked for": L.hf_depthwise_k_grad(10, 8, 64, 1, fake, fake, fake, None, None, None),
        "depthwise grad: rows < 0": L.hf_depthwise_k_grad(-1, 8, 64, 1, fake, fake, fake, fake, fake, None),
    }
    wrong = {name: got for name, got in bad.items() if got != EINVAL}
    assert not wrong, wrong
    need = L.hf_xconv_depthwise_gather_grad_workspace(2, 7, 8, 64, 36, 1)
    assert need == xc.gather_grad_workspace(2, 7, 8, 64, 36, 1) > 0
    assert gather_grad(ws=fake, nbytes=need - 1) == EWS
    need = L.hf_depthwise_k_grad_workspace(203, 8, 640, 2)
    assert need == xc.dw_grad_workspace(203, 8, 640, 2)
    assert L.hf_depthwise_k_grad_ws(203, 8, 640, 2, fake, fake, fake, None, fake, fake, need - 1, None) == EWS
    assert L.hf_depthwise_k_grad_ws(203, 8, 640, 2, fake, fake, fake, None, fake, None, big, None) == EWS
    assert L.hf_xconv_depthwise_gather_grad_workspace(0, 7, 8, 64, 36, 1) == 0 and L.hf_depthwise_k_grad_workspace(0, 8, 8, 8) == 0
    # the restated workspace sizes at every case that takes one
    for c in CASES:
        if c["kind"] == "bwd" and c["gather"]:
            assert L.hf_xconv_depthwise_gather_grad_workspace(c["b"], c["p"], c["k"], c["c0"], c["c1"], c["m"]) == xc.gather_grad_workspace(
                c["b"], c["p"], c["k"], c["c0"], c["c1"], c["m"]), xc.case_id(c)
        if c["kind"] == "dw_grad":
            assert L.hf_depthwise_k_grad_workspace(c["rows"], c["k"], c["c"], c["m"]) == xc.dw_grad_workspace(c["rows"], c["k"], c["c"], c["m"]), xc.case_id(c)
