"""Every launch regime of the FPS, ball-query, kNN and select_top_k kernels on the GPU against the project's CPU oracle, parametrized over
the case table of tests/geometry_cases.py (which restates the dispatch, and whose CPU tests check the oracle against an independent NumPy
statement and that the cases reach every compiled instantiation).  The Python wrappers are called where they expose the selector
(farthest_point_sample(kernel=, threads=), query_ball_point / query_ball_group(variant=), knn_point(all_pairs=), three_nn); _lib.lib()
is called directly for what they do not expose: a cloud pointer 4 bytes past a 16-byte boundary and an explicit workspace for the
auto -> cell-sorted route.  Picks, indices, counts, grouped coordinates and kNN distances are compared with np.array_equal: the outputs
are integers, copies and fp32 expressions without contraction, with a deterministic tie rule.  The forced call of every case must also
equal the automatic choice on the same inputs."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_cases as gc  # noqa: E402
from abi_harness import dev, host, same_array  # noqa: E402

pytestmark = pytest.mark.gpu

IDX_SENTINEL = -7
DEV = "cuda"


@pytest.fixture(scope="module")
def hf():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import heterofusionrcnn_amd as m
    return m


def same(got, want, what, c):
    same_array(got, want, what, gc.case_id(c))


# ---------------------------------------------------------------------------------------------- farthest point sampling
@pytest.mark.parametrize("c", gc.cases_of("fps"), ids=gc.case_id)
def test_geometry_fps(hf, oracle_mod, c):
    t = gc.make_inputs(c)
    want = gc.oracle_outputs(c, t, oracle_mod)["out"]
    x = dev(DEV, t["xyz"])
    got = hf.farthest_point_sample(c["m"], x, kernel=c["kernel"], threads=c["threads"])
    same(got, want, "picks", c)
    same(hf.farthest_point_sample(c["m"], x), want, "picks of the automatic choice", c)


# ---------------------------------------------------------------------------------------------- ball query
def _ball_query_abi(c, t):
    """hf_query_ball_group_xyz_ws called directly: the cloud 4 bytes past a 16-byte boundary (off), an explicit workspace (ws); the
    outputs are pre-filled, so an element that is never written shows"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    b, n, m, ns = c["b"], c["n"], c["m"], c["nsample"]
    start = 1 if c["off"] else 0
    buf = torch.full((start + b * n * 3 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    buf[start:start + b * n * 3].copy_(torch.from_numpy(t["xyz1"].reshape(-1)))
    x1 = ctypes.c_void_p(buf.data_ptr() + 4 * start)
    assert x1.value % 16 == (4 if c["off"] else 0)
    x2 = dev(DEV, t["xyz2"])
    idx = torch.full((b, m, ns), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((b, m), IDX_SENTINEL, dtype=torch.int32, device="cuda")
    grouped = torch.full((b, m, ns, 3), float("nan"), dtype=torch.float32, device="cuda") if c["group"] else None
    ws, nbytes = None, 0
    if c["ws"]:
        nbytes = L.hf_ball_query_workspace(b, n)
        assert nbytes == gc.sorted_workspace(b, n)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        assert ws.data_ptr() % 16 == 0
    _lib.check(L.hf_query_ball_group_xyz_ws(gc.BQ_VARIANTS.index(c["variant"]), b, n, m, c["radius"], ns, x1, _lib.ptr(x2), 1 if c["center"] else 0,
                                            _lib.ptr(idx), _lib.ptr(cnt), _lib.ptr(grouped), _lib.ptr(ws), nbytes, _lib.stream_ptr()), "query_ball_group_xyz_ws")
    torch.cuda.synchronize()
    assert torch.isnan(buf[start + b * n * 3:]).all() and (start == 0 or bool(torch.isnan(buf[0])))
    return idx, cnt, grouped


def _ball_query_wrapper(hf, c, t, variant):
    x1, x2 = dev(DEV, t["xyz1"]), dev(DEV, t["xyz2"])
    if c["group"]:
        return hf.query_ball_group(c["radius"], c["nsample"], x1, x2, center=c["center"], variant=variant)
    return hf.query_ball_point(c["radius"], c["nsample"], x1, x2, variant=variant) + (None,)


@pytest.mark.parametrize("c", gc.cases_of("bq"), ids=gc.case_id)
def test_geometry_ball_query(hf, oracle_mod, c):
    t = gc.make_inputs(c)
    want = gc.oracle_outputs(c, t, oracle_mod)
    legs = [("forced", _ball_query_abi(c, t) if (c["off"] or c["ws"]) else _ball_query_wrapper(hf, c, t, c["variant"])),
            ("the automatic choice", _ball_query_wrapper(hf, c, t, "auto"))]
    for leg, (idx, cnt, grouped) in legs:
        same(idx, want["idx"], "idx, " + leg, c)
        same(cnt, want["cnt"], "pts_cnt, " + leg, c)
        if c["group"]:
            same(grouped, want["grouped"], "grouped_xyz, " + leg, c)


# ---------------------------------------------------------------------------------------------- kNN, three_nn, select_top_k
@pytest.mark.parametrize("c", gc.cases_of("knn"), ids=gc.case_id)
def test_geometry_knn(hf, oracle_mod, c):
    t = gc.make_inputs(c)
    want = gc.oracle_outputs(c, t, oracle_mod)
    x1, x2 = dev(DEV, t["xyz1"]), dev(DEV, t["xyz2"])
    if c["entry"] == "three_nn":
        val, idx = hf.three_nn(x2, x1)            # (unknown, known)
    else:
        val, idx = hf.knn_point(c["k"], x1, x2, all_pairs=c["entry"] == "all_pairs")
    same(idx, want["idx"], "idx", c)
    same(val, want["val"], "distances", c)
    assert (np.diff(host(val), axis=-1) >= 0).all()
    v2, i2 = hf.knn_point(c["k"], x1, x2)         # the wrapper's own choice between the two entry points
    same(i2, want["idx"], "idx of the automatic choice", c)
    same(v2, want["val"], "distances of the automatic choice", c)


@pytest.mark.parametrize("c", gc.cases_of("topk"), ids=gc.case_id)
def test_geometry_select_top_k(hf, oracle_mod, c):
    t = gc.make_inputs(c)
    want = gc.oracle_outputs(c, t, oracle_mod)
    outi, out = hf.select_top_k(c["k"], dev(DEV, t["dist"]))
    same(outi, want["outi"], "indices", c)
    same(out, want["out"], "distances", c)
