"""hf_compute_bev_iou, hf_nms_mask, hf_oriented_nms and hf_oriented_nms_batched (csrc/bev_iou.hip) on the GPU, through _lib.lib() and
ctypes with no Python routing in between, against the fp64 statements of tests/bev_cases.py: the Sutherland-Hodgman clip for the
values, the greedy sweep over the sparse fp64 adjacency for keep / num_kept, in every regime of the sweep the case table reaches
(tests/test_bev_cases_cpu.py shows that it does).

Every output is pre-filled with a sentinel (NaN for floats, -7 for ints, a byte pattern for mask words) and none may survive; the
workspace is exactly frames * hf_oriented_nms_workspace(n) bytes between guard bytes that must be intact after the call.

BEV_CASES_OUT=<file>: the device-side figures of profiles/bev_cases.md (wall times, the decisions on the excluded pairs of the
equal-heading family) as JSON lines."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bev_cases as bc  # noqa: E402
from abi_harness import Workspace, abi, dev, host  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5                     # test_ops_gpu.TOL: device against the fp32 oracle
MASK_FILL = 0x5A5A5A5A5A5A5A5A

# established regimes first, the streaming sweep's wrapped rings after them, the largest last
ORDER = ["G%d" % n for n in bc.G_SIZES] + ["D", "E", "Cs", "C", "B", "F"]
NMS_IDS = [(name, t) for name in ORDER for t in bc.NMS_CASES[name]["thresh"]]
assert sorted(NMS_IDS) == sorted(bc.nms_case_ids())
_id = lambda p: "%s-%g" % p


def record(**kw):
    print("\n" + json.dumps(kw))
    if os.environ.get("BEV_CASES_OUT"):
        with open(os.environ["BEV_CASES_OUT"], "a") as f:
            f.write(json.dumps(kw) + "\n")


def run_nms(boxes_dev, frames, n, thresh, batched):
    """one call into fresh, sentinel-filled buffers -> (keep (frames, n), num_kept (frames,)) on the host, seconds"""
    _lib, L = abi()
    nbytes = frames * L.hf_oriented_nms_workspace(n)
    assert L.hf_oriented_nms_workspace(n) >= 8 * n * ((n + 63) // 64)
    keep = torch.full((frames, n), bc.SENT_I, dtype=torch.int32, device="cuda")
    num = torch.full((frames,), bc.SENT_I, dtype=torch.int32, device="cuda")
    ws = Workspace(DEV, nbytes)
    args = (_lib.ptr(boxes_dev), n, thresh, _lib.ptr(keep), _lib.ptr(num))
    call = (lambda *tail: L.hf_oriented_nms_batched(frames, *args, *tail)) if batched else (lambda *tail: L.hf_oriented_nms(*args, *tail))
    # one byte short: refused before anything is launched (nothing written)
    assert call(ws.p, nbytes - 1, _lib.stream_ptr()) == bc.HF_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((keep == bc.SENT_I).all()) and bool((num == bc.SENT_I).all())
    t0 = time.perf_counter()
    _lib.check(call(ws.p, nbytes, _lib.stream_ptr()), "oriented_nms")
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    ws.check("hf_oriented_nms n=%d" % n)
    return host(keep), host(num), seconds


def check_keep(keep, num, want_keep, want_kept, what):
    assert not (num == bc.SENT_I).any() and not (keep == bc.SENT_I).any(), "%s: %d elements of keep never written" % (what, int((keep == bc.SENT_I).sum()))
    assert int(num) == want_kept, "%s: num_kept %d, want %d" % (what, int(num), want_kept)
    if not np.array_equal(keep, want_keep):
        bad = np.flatnonzero(keep != want_keep)
        raise AssertionError("%s: keep differs at %d of %d positions, the first at %d: got %d, want %d"
                             % (what, len(bad), len(keep), bad[0], keep[bad[0]], want_keep[bad[0]]))
    assert (keep[want_kept:] == keep[0]).all() and keep[0] == 0


# ------------------------------------------------------------------------------------------------ bad arguments: no launch
def test_bad_arguments_are_refused_before_any_launch():
    _lib, L = abi()
    one, big = ctypes.c_void_p(4096), 1 << 60           # never dereferenced: the checks come first
    EINVAL, EWS = bc.HF_EINVAL, bc.HF_EWORKSPACE
    nms = lambda n, t, keep=one, boxes=one, ws=one, nbytes=big: L.hf_oriented_nms(boxes, n, t, keep, one, ws, nbytes, None)
    bat = lambda f, n, t, keep=one, ws=one, nbytes=big: L.hf_oriented_nms_batched(f, one, n, t, keep, one, ws, nbytes, None)
    for n in (0, -1):
        assert nms(n, 0.5) == EINVAL and bat(2, n, 0.5) == EINVAL and L.hf_oriented_nms_workspace(n) == 0
    for f in (0, -1, bc.MAX_FRAMES + 1):
        assert bat(f, 64, 0.5) == EINVAL, f
    for t in (-0.1, -1e-30, float("nan")):
        assert nms(64, t) == EINVAL and bat(2, 64, t) == EINVAL, t
    assert nms(64, 0.5, keep=None) == EINVAL and bat(2, 64, 0.5, keep=None) == EINVAL and nms(64, 0.5, boxes=None) == EINVAL
    need = L.hf_oriented_nms_workspace(64)
    assert need > 0 and nms(64, 0.5, ws=None) == EWS and nms(64, 0.5, nbytes=need - 1) == EWS and bat(3, 64, 0.5, nbytes=3 * need - 1) == EWS
    assert nms(64, 0.5, ws=ctypes.c_void_p(4096 + 8)) == EINVAL and bat(2, 64, 0.5, ws=ctypes.c_void_p(4096 + 4)) == EINVAL
    too_many = bc.MAX_SWEEP_BLOCKS * 64 + 1
    assert nms(too_many, 0.5) == EINVAL and bat(2, too_many, 0.5) == EINVAL
    assert L.hf_oriented_nms_workspace(bc.MAX_SWEEP_BLOCKS * 64) > 0
    # hf_nms_mask
    mask = lambda n, boxes=one, out=one: L.hf_nms_mask(boxes, out, n, 0.5, None)
    assert mask(0) == EINVAL and mask(-5) == EINVAL and mask(64, boxes=None) == EINVAL and mask(64, out=None) == EINVAL
    assert mask(65535 * 64 + 1) == EINVAL
    # hf_compute_bev_iou
    iou = lambda na, nb, a=one, b=one, ov=one, io=one: L.hf_compute_bev_iou(na, a, nb, b, ov, io, None)
    assert iou(0, 3) == EINVAL and iou(3, 0) == EINVAL and iou(-1, 3) == EINVAL and iou(3, 3, a=None) == EINVAL and iou(3, 3, b=None) == EINVAL
    assert iou(3, 3, ov=None, io=None) == bc.HF_OK                     # nothing asked for, nothing launched
    for off in (4, 8, 12):
        bad = ctypes.c_void_p(4096 + off)
        assert iou(3, 3, ov=bad) == EINVAL and iou(3, 3, io=bad) == EINVAL and iou(3, 3, ov=bad, io=None) == EINVAL and iou(3, 3, ov=None, io=bad) == EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ hf_oriented_nms
@pytest.mark.parametrize("case", NMS_IDS, ids=_id)
def test_oriented_nms(case):
    name, thresh = case
    fx, m = bc.nms_fixture(name), bc.nms_model(name, thresh)
    boxes = dev(DEV, fx["boxes"])
    what = "%s at %g (%s)" % (name, thresh, m["regime"])
    keep, num, seconds = run_nms(boxes, 1, m["n"], thresh, batched=False)
    check_keep(keep[0], num[0], m["keep"], m["kept"], what)
    keep2, num2, seconds2 = run_nms(boxes, 1, m["n"], thresh, batched=False)
    assert keep.tobytes() == keep2.tobytes() and num.tobytes() == num2.tobytes(), "%s: a second call gives other bytes" % what
    if name == "F":
        record(case=name, n=m["n"], seconds_first=round(seconds, 4), seconds_second=round(seconds2, 4))


def test_oriented_nms_batched_frames_take_different_forms():
    frames = bc.batch_frames()
    n = len(frames[0][0])
    boxes = dev(DEV, np.stack([b for b, _ in frames]))
    for again in range(2):
        keep, num, _ = run_nms(boxes, len(frames), n, bc.BATCH_THRESH, batched=True)
        for f, (_, m) in enumerate(frames):
            check_keep(keep[f], num[f], m["keep"], m["kept"], "frame %d (%s)" % (f, m["regime"]))
    assert len({int(v) for v in num}) == len(frames)


# ------------------------------------------------------------------------------------------------ hf_nms_mask
def run_mask(boxes, thresh):
    _lib, L = abi()
    n = len(boxes)
    cb = (n + 63) // 64
    guarded = torch.full((n * cb + 64,), MASK_FILL, dtype=torch.int64, device="cuda")
    out = guarded[32:32 + n * cb]
    _lib.check(L.hf_nms_mask(_lib.ptr(dev(DEV, boxes)), ctypes.c_void_p(out.data_ptr()), n, thresh, _lib.stream_ptr()), "nms_mask")
    torch.cuda.synchronize()
    assert bool((guarded[:32] == MASK_FILL).all()) and bool((guarded[32 + n * cb:] == MASK_FILL).all()), "written outside the mask"
    return host(out).view(np.uint64).reshape(n, cb)


MASK_IDS = [(name, t, None) for name in ORDER if name.startswith("G") for t in bc.G_THRESH] + [("C", 0.1, 1024)]


@pytest.mark.parametrize("case", MASK_IDS, ids=lambda p: "%s-%g" % p[:2])
def test_nms_mask(case):
    name, thresh, cut = case
    m = bc.nms_model(name, thresh, cut)
    got = run_mask(bc.nms_fixture(name)["boxes"][:m["n"]], thresh)
    want = bc.dense_mask(m["n"], m["ai"], m["aj"])
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s at %g: %d of %d words differ, the first at %s: got %#x, want %#x"
                             % (name, thresh, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------------ hf_compute_bev_iou
_BOUND = []


def bound(oracle_mod):
    """the value bound: sampler_cases.iou_bound's rule on the largest |fp32 oracle - fp64 clip| over every same-site pair of every
    generic-heading case (tests/test_bev_cases_cpu.py prints the terms and checks the margin of the fixtures against it)"""
    if not _BOUND:
        err = max([bc.oracle_site_error(oracle_mod, bc.nms_fixture(name))[0] for name in bc.NMS_CASES] +
                  [bc.oracle_site_error(oracle_mod, bc.iou_case(name)["fx"])[0] for name in bc.iou_case_ids() + ["slab"]])
        _BOUND.append(bc.value_bound(err))
        print("\nlargest |oracle - fp64| %.3g -> bound %.3g" % (err, _BOUND[0]))
    return _BOUND[0]


def run_iou(a, b, with_ov, with_iou):
    _lib, L = abi()
    na, nb = len(a), len(b)
    outs = [torch.full((na * nb + 8,), float("nan"), dtype=torch.float32, device="cuda") if use else None for use in (with_ov, with_iou)]
    views = [o[4:4 + na * nb] if o is not None else None for o in outs]           # 16 bytes in: still aligned
    _lib.check(L.hf_compute_bev_iou(na, _lib.ptr(a), nb, _lib.ptr(b), _lib.ptr(views[0]), _lib.ptr(views[1]), _lib.stream_ptr()), "compute_bev_iou")
    torch.cuda.synchronize()
    for o in outs:
        if o is not None:
            assert bool(o[:4].isnan().all()) and bool(o[4 + na * nb:].isnan().all()), "written outside the output"
    return [v.view(na, nb) if v is not None else None for v in views]


@pytest.mark.parametrize("name", bc.iou_case_ids())
def test_compute_bev_iou(oracle_mod, name):
    c = bc.iou_case(name)
    a, b = dev(DEV, c["a"]), dev(DEV, c["b"])
    ov_d, iou_d = run_iou(a, b, True, True)
    ov, iou = host(ov_d), host(iou_d)
    assert not np.isnan(ov).any() and not np.isnan(iou).any(), "%d / %d elements never written" % (int(np.isnan(ov).sum()), int(np.isnan(iou).sum()))
    same = np.zeros((c["na"], c["nb"]), bool)
    same[c["rows"], c["cols"]] = True
    # cross-site pairs: exact zeros in both outputs
    assert (ov[~same] == 0).all() and (iou[~same] == 0).all(), "%d nonzero cross-site overlaps" % int((ov[~same] != 0).sum())
    assert np.array_equal(ov == 0, iou == 0), "the two outputs do not share their zero pattern"
    # same-site pairs against the fp64 clip
    bd = bound(oracle_mod)
    e_iou = np.abs(iou[c["rows"], c["cols"]].astype(np.float64) - c["iou"])
    larger = np.maximum(bc.areas(c["a"])[c["rows"]], bc.areas(c["b"])[c["cols"]])
    e_ov = np.abs(ov[c["rows"], c["cols"]].astype(np.float64) - c["ov"]) / larger
    print("\n%s: %d same-site pairs, |iou - fp64| <= %.3g, |overlap - fp64| / area <= %.3g, bound %.3g" % (name, len(e_iou), e_iou.max(), e_ov.max(), bd))
    assert (e_iou <= bd).all(), (e_iou.max(), bd)
    assert (e_ov <= bd).all(), (e_ov.max(), bd)
    # ... and the fp32 oracle at the tolerance of test_ops_gpu
    o_ov, o_iou = oracle_mod.compute_bev_iou(c["a"], c["b"])
    np.testing.assert_allclose(iou, o_iou, rtol=0, atol=TOL)
    if name == "dense":
        assert (iou > 0).all() and same.all()
    # one output alone: the same bytes
    only_ov, none = run_iou(a, b, True, False)
    assert none is None and host(only_ov).tobytes() == ov.tobytes(), "overlap alone differs from the two-output call"
    none, only_iou = run_iou(a, b, False, True)
    assert none is None and host(only_iou).tobytes() == iou.tobytes(), "IoU alone differs from the two-output call"


def test_compute_bev_iou_slab_walk(oracle_mod):
    """more row tiles than one grid holds: planted rows on both sides of the slab boundary, zeros everywhere else"""
    c = bc.iou_case("slab")
    na, nb = bc.SLAB_SHAPE
    a, b = torch.from_numpy(bc.slab_rows()).cuda(), dev(DEV, c["b"])
    planted = torch.tensor(bc.SLAB_PLANTED, device="cuda")
    bd = bound(oracle_mod)
    want_iou, want_ov = c["iou"].reshape(len(bc.SLAB_PLANTED), nb), c["ov"].reshape(len(bc.SLAB_PLANTED), nb)
    assert np.array_equal(c["rows"], np.repeat(np.arange(len(bc.SLAB_PLANTED)), nb)) and np.array_equal(c["cols"], np.tile(np.arange(nb), len(bc.SLAB_PLANTED)))
    first = {}
    for with_ov, with_iou in ((True, True), (True, False), (False, True)):
        t0 = time.perf_counter()
        ov_d, iou_d = run_iou(a, b, with_ov, with_iou)
        seconds = time.perf_counter() - t0
        for key, out, want, scale in (("overlap", ov_d, want_ov, bc.areas(c["a"]).max()), ("iou", iou_d, want_iou, 1.0)):
            if out is None:
                continue
            rows = out[planted]
            # on the device: every element written, nothing nonzero outside the planted rows (NaN counts as nonzero)
            assert int(torch.count_nonzero(out)) == int(torch.count_nonzero(rows)) == rows.numel(), key
            got = host(rows)
            err = np.abs(got.astype(np.float64) - want) / scale
            assert (err <= bd).all(), (key, err.max(), bd)
            if key in first:
                assert got.tobytes() == first[key].tobytes(), "%s alone differs from the two-output call" % key
            first.setdefault(key, got)
        if with_ov and with_iou:
            record(case="slab", num_a=na, num_b=nb, seconds=round(seconds, 4))


# ------------------------------------------------------------------------------------------------ the equal-heading family
@pytest.mark.parametrize("name", bc.equal_case_ids())
def test_nms_mask_equal_headings(oracle_mod, name):
    """parallel edges: the device's mask equals the fp32 oracle's wherever the oracle agrees with the closed form about
    `iou > thresh`; the pairs where it does not are counted, and which way the device went"""
    c = bc.equal_case(name)
    di, dj, closed, pairs, want = bc.equal_disagreement(oracle_mod, name)
    assert len(di) < bc.EQUAL_CAP * pairs
    got = run_mask(c["boxes"], bc.EQUAL_THRESH)
    excluded = np.zeros_like(want)
    for i, j in ((di, dj), (dj, di)):
        np.bitwise_or.at(excluded, (i, j // 64), np.uint64(1) << (j % 64).astype(np.uint64))
    differ = (got ^ want) & ~excluded
    assert not differ.any(), "%d words differ from the oracle outside the excluded pairs, the first at %s" % (int(differ.astype(bool).sum()), tuple(np.argwhere(differ)[0]))
    bit = ((got[di, dj // 64] >> (dj % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
    record(case=name, overlapping_pairs=pairs, excluded=len(di), device_as_closed_form=int((bit == closed).sum()), device_as_oracle=int((bit != closed).sum()))
