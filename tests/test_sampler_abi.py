"""The RPN batch sampler (csrc/rpn_batch.hip) and the RCNN target layer (csrc/rcnn_targets.hip) on the GPU, draw for draw against the NumPy
restatement of tests/sampler_cases.py, through _lib.lib() and ctypes with no Python routing in between.

Both files draw from a pure integer counter hash and the library is built with -ffp-contract=off, so the sampled indices, the status
words, the rng_state, the labels, the images and every fp32 output made of + - * / are compared with np.array_equal.  What goes through
the device's transcendental functions is held to a bound measured on the host at run time, never against the kernel: the 3D IoU to
ELU_FACTOR x the error of the float32 CPU form against the fp64 clip, the 'normal' jitter to ELU_FACTOR x the error of a float32 NumPy
evaluation against its float64 evaluation, the image noise vector to 1e-12 relative.

Every output is pre-filled with a sentinel (NaN for floats, -7 for ints) and none may survive; every workspace is exactly the size its
*_workspace entry point reports, carved out of a larger buffer whose guard bytes on both sides must be intact after the call.  The forced
C-ABI call of every case must equal the Python wrapper on the same inputs, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402
from abi_harness import Workspace, abi, dev, filled, host, same_array  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
RATIOS = {"iou": 0.0, "normal": 0.0}


def same(got, want, what, c):
    same_array(got, want, what, sc.case_id(c), unwritten=sc.SENT_I)


def same_bits(a, b, what, c):
    a, b = host(a), host(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s of %s: the C-ABI call and the wrapper differ" % (what, sc.case_id(c))


@pytest.fixture(scope="module", autouse=True)
def ratio_report():
    yield
    print("\nlargest observed error / bound: 3D IoU %.3g, 'normal' jitter %.3g" % (RATIOS["iou"], RATIOS["normal"]))


# ---------------------------------------------------------------------------------------------- RPN points
@pytest.mark.parametrize("c", sc.cases_of("points"), ids=sc.case_id)
def test_rpn_batch_points(c):
    from heterofusionrcnn_amd import kitti_data as KD
    _lib, L = abi()
    t = sc.make_inputs(c)
    b, p, total, mx = len(c["frames"]), c["p"], t["total"], t["max_frame"]
    ins = [dev(DEV, t[k]) for k in ("points", "offsets", "velo_to_rect", "p2", "wh", "flip")]
    state, wstate = dev(DEV, t["state"]), dev(DEV, t["state"])
    nbytes = L.hf_rpn_batch_points_workspace(b, total, mx)
    assert nbytes == sc.rpn_points_workspace(b, total, mx) and nbytes % 256 == 0
    for call in range(c["calls"]):
        want = sc.ref_rpn_points(c, t, call)
        xyz, inten = filled(DEV, (b, p, 3), torch.float32, sc.SENT_I), filled(DEV, (b, p, 1), torch.float32, sc.SENT_I)
        src, status = filled(DEV, (b, p), torch.int32, sc.SENT_I), filled(DEV, (b,), torch.int32, sc.SENT_I)
        ws = Workspace(DEV, nbytes)
        _lib.check(L.hf_rpn_batch_points(b, p, total, mx, *[_lib.ptr(x) for x in ins], _lib.ptr(state), _lib.ptr(xyz), _lib.ptr(inten),
                                         _lib.ptr(src), _lib.ptr(status), ws.p, nbytes, _lib.stream_ptr()), "rpn_batch_points")
        ws.check("hf_rpn_batch_points")
        same(src, want[2], "src_index (call %d)" % call, c)
        same(status, want[3], "status", c)
        same(xyz, want[0], "xyz", c)
        same(inten, want[1], "intensity", c)
        same(state, want[4], "rng_state after call %d" % call, c)
        got = KD.batch_points(*ins, wstate, p, mx)
        for a, w, name in zip((xyz, inten, src, status), got, ("xyz", "intensity", "src_index", "status")):
            same_bits(a, w, name, c)
        same_bits(state, wstate, "rng_state", c)


# ---------------------------------------------------------------------------------------------- RPN labels
@pytest.mark.parametrize("c", sc.cases_of("labels"), ids=sc.case_id)
def test_rpn_point_labels(c):
    from heterofusionrcnn_amd import kitti_data as KD
    _lib, L = abi()
    t = sc.make_inputs(c)
    b, p, g = c["b"], c["p"], c["g"]
    want_cls, want_reg, _ = sc.ref_rpn_labels(c, t)
    xyz, boxes, classes, cnt = dev(DEV, t["xyz"]), dev(DEV, t["boxes"]), dev(DEV, t["classes"]), dev(DEV, t["gt_count"])
    cls, reg = filled(DEV, (b, p), torch.int32, sc.SENT_I), filled(DEV, (b, p, 7), torch.float32, sc.SENT_I)
    _lib.check(L.hf_rpn_point_labels(b, p, g, _lib.ptr(xyz), _lib.ptr(boxes) if g else None, _lib.ptr(classes) if g else None, _lib.ptr(cnt),
                                     float(c["expand"]), _lib.ptr(cls), _lib.ptr(reg), _lib.stream_ptr()), "rpn_point_labels")
    torch.cuda.synchronize()
    got_cls = host(cls)
    assert got_cls.min() >= -1, "a label was never written"
    assert np.array_equal(got_cls, want_cls), (sc.case_id(c), np.argwhere(got_cls != want_cls)[:5].tolist())
    same(reg, want_reg, "label_reg", c)
    w_cls, w_reg = KD.point_labels(xyz, boxes, classes, cnt, c["expand"])
    same_bits(cls, w_cls, "label_cls", c)
    same_bits(reg, w_reg, "label_reg", c)


# ---------------------------------------------------------------------------------------------- image
@pytest.mark.parametrize("c", sc.cases_of("image"), ids=sc.case_id)
def test_rpn_batch_image(c):
    from heterofusionrcnn_amd import kitti_data as KD
    _lib, L = abi()
    t = sc.make_inputs(c)
    b = len(c["frames"])
    ow, oh = c["out"]
    ins = [dev(DEV, t[k]) for k in ("images", "offsets", "wh", "flip", "jitter")]
    state, wstate = dev(DEV, t["state"]), dev(DEV, t["state"])
    nbytes = L.hf_rpn_batch_image_workspace(b, t["max_pixels"])
    assert nbytes == sc.rpn_image_workspace(b, t["max_pixels"])
    for call in range(c["calls"]):
        image, noise, stats = filled(DEV, (b, oh, ow, 3), torch.float32, sc.SENT_I), filled(DEV, (b, 3), torch.float64, sc.SENT_I), filled(DEV, (b, 21), torch.float64, sc.SENT_I)
        ws = Workspace(DEV, nbytes)
        _lib.check(L.hf_rpn_batch_image(b, t["max_pixels"], len(t["images"]), *[_lib.ptr(x) for x in ins], oh, ow, _lib.ptr(state),
                                        _lib.ptr(image), _lib.ptr(noise), _lib.ptr(stats), ws.p, nbytes, _lib.stream_ptr()), "rpn_batch_image")
        ws.check("hf_rpn_batch_image")
        got_noise, got_stats = host(noise), host(stats)
        assert not np.isnan(got_noise).any() and not np.isnan(got_stats).any(), "a noise or stats element was never written"
        want_image, want_noise, want_state, info = sc.ref_image(c, t, call, stats=got_stats, noise=got_noise)
        tol = max(1e-12 * float(np.abs(want_noise).max()), 1e-15)
        err = float(np.abs(got_noise - want_noise).max())
        assert err <= tol, "%s: the noise vector is %.3g off the restated formula (bound %.3g)" % (sc.case_id(c), err, tol)
        for f, kind in enumerate(info["kind"]):
            if kind == "invalid" or "one_pixel" in kind or "zero_cov" in kind or not kind.startswith("jitter"):
                assert not got_noise[f].any(), (kind, got_noise[f])
            else:
                assert np.abs(got_noise[f]).max() > 0
                # the e, v of the stats are an eigendecomposition of the exact covariance (tests/test_kitti_data.py holds them to eigh too)
                e, v = got_stats[f, 9:12], got_stats[f, 12:21].reshape(3, 3)
                cov = sc.KN.covariance(t["frames"][f])
                np.testing.assert_allclose(cov @ v, v * e, rtol=0, atol=1e-12 * np.abs(cov).max())
        same(image, want_image, "image (call %d)" % call, c)
        same(state, want_state, "rng_state", c)
        w_image, w_noise, w_stats = KD.batch_image(*ins, wstate, (oh, ow), t["max_pixels"], stats=True)
        same_bits(image, w_image, "image", c)
        same_bits(noise, w_noise, "noise", c)
        same_bits(stats, w_stats, "pca stats", c)
        same_bits(state, wstate, "rng_state", c)


# ---------------------------------------------------------------------------------------------- RCNN targets
def _targets_call(c, t, state, ws):
    _lib, L = abi()
    b, m, g, r = c["b"], c["m"], c["g"], c["r"]
    ins = t["dev"]
    rois, iou, gt_of = filled(DEV, (b, r, 7), torch.float32, sc.SENT_I), filled(DEV, (b, r), torch.float32, sc.SENT_I), filled(DEV, (b, r, 8), torch.float32, sc.SENT_I)
    stats = filled(DEV, (b, 4), torch.int32, sc.SENT_I)
    f32 = lambda v: float(np.float32(v))
    _lib.check(L.hf_rcnn_proposal_targets(b, m, g, _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]) if g else None, _lib.ptr(ins[3]),
                                          f32(c["neg"][0]), f32(c["neg"][1]), f32(c["pos"][0]), f32(c["pos"][1]), r, f32(c["fg_ratio"]),
                                          f32(c["hard_ratio"]), sc.aug_code(c), c["train"], _lib.ptr(state) if c["train"] else None,
                                          _lib.ptr(rois), _lib.ptr(iou), _lib.ptr(gt_of), _lib.ptr(stats), ws.p, ws.nbytes,
                                          _lib.stream_ptr()), "rcnn_proposal_targets")
    ws.check("hf_rcnn_proposal_targets")
    return rois, iou, gt_of, stats


def _config(c):
    from heterofusionrcnn_amd import rcnn_train as RT
    return RT.RcnnTrainConfig(cls_neg_iou_range=c["neg"], cls_pos_iou_range=(c["pos"][0], 1.0), reg_pos_iou_range=(c["pos"][1], 1.0),
                              roi_per_sample=c["r"], fg_ratio=c["fg_ratio"], hard_bg_ratio=c["hard_ratio"])


def normal_bound(want32, want64, src, max_normal):
    """per element ELU_FACTOR x |float32 NumPy evaluation - float64 evaluation|, floored at U (|in| + sigma max|r|)"""
    sigma = np.array([0.3, 0.2, 0.3, 0.25, 0.15, 0.5, np.pi / 12])
    r = np.array([max_normal] * 6 + [1.0])
    floor = sc.U * (np.abs(src.astype(np.float64)) + sigma * r)
    return np.maximum(sc.ELU_FACTOR * np.abs(want32.astype(np.float64) - want64), floor)


@pytest.mark.parametrize("c", sc.cases_of("targets"), ids=sc.case_id)
def test_rcnn_proposal_targets(c, oracle_mod):
    from heterofusionrcnn_amd import rcnn_train as RT
    _lib, L = abi()
    t = dict(sc.make_inputs(c))
    b, m, g, r = c["b"], c["m"], c["g"], c["r"]
    t["dev"] = [dev(DEV, t[k]) for k in ("proposals", "proposal_count", "gt", "gt_count")]
    state, wstate = dev(DEV, t["state"]), dev(DEV, t["state"])
    nbytes = L.hf_rcnn_targets_workspace(b, m, g)
    assert nbytes == sc.rcnn_targets_workspace(b, m, g)
    aug = sc.aug_code(c)
    for call in range(c["calls"]):
        want = sc.ref_rcnn_targets(c, t, call)
        rois, iou, gt_of, stats = _targets_call(c, t, state, Workspace(DEV, nbytes))
        same(stats, want["stats"], "stats (call %d)" % call, c)
        same(gt_of, want["gt_of_rois"], "gt_of_rois", c)
        if c["train"]:
            same(state, want["state"], "rng_state", c)
        if aug != 3:
            same(rois, want["rois"], "rois", c)
        else:
            got = host(rois)
            assert not np.isnan(got).any(), "a roi was never written"
            moved = want["info"]["moved"]
            assert np.array_equal(got[~moved], want["rois"][~moved]), "a RoI that no try moved is not the proposal's bits"
            bound = normal_bound(want["rois"], want["rois64"], want["src"], want["info"]["max_normal"])
            err = np.abs(got.astype(np.float64) - want["rois64"])
            assert (err[bound == 0] == 0).all(), "a roi of a frame without proposals is not 0.0"
            ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
            RATIOS["normal"] = max(RATIOS["normal"], ratio)
            print("'normal' jitter of %s: largest error / bound %.3g (largest error %.3g)" % (sc.case_id(c), ratio, float(err.max())))
            assert (err <= bound).all(), "%s: rois under 'normal' %.3g x the bound at %s" % (sc.case_id(c), ratio, np.argwhere(err > bound)[:3].tolist())
        bound, measured = sc.iou_bound(c, t, oracle_mod, want["info"]["pairs"])
        got_iou = host(iou)
        assert not np.isnan(got_iou).any(), "an iou_of_rois element was never written"
        err = float(np.abs(got_iou.astype(np.float64) - want["iou"]).max())
        RATIOS["iou"] = max(RATIOS["iou"], err / bound)
        print("iou_of_rois of %s: error %.3g, bound %.3g (float32 CPU form %.3g off fp64)" % (sc.case_id(c), err, bound, measured))
        assert err <= bound, "%s: iou_of_rois %.3g off fp64, bound %.3g" % (sc.case_id(c), err, bound)
        still = ~want["info"]["moved"]
        assert (got_iou[still & (want["iou"] == 0)] == 0).all(), "an IoU that is exactly 0 (disjoint boxes, zero padding) is not 0.0"
        w = RT.proposal_targets(*t["dev"], wstate if c["train"] else None, _config(c), train=bool(c["train"]), aug_method=c["aug"])
        for a, x, name in zip((rois, iou, gt_of, stats), w, ("rois", "iou_of_rois", "gt_of_rois", "stats")):
            same_bits(a, x, name, c)
        if c["train"]:
            same_bits(state, wstate, "rng_state", c)


@pytest.mark.parametrize("c", [c for c in sc.cases_of("targets") if c["calls"] == 1 and (c["train"] or c["g"] == 0)], ids=sc.case_id)
def test_box3d_iou_matrix(c, oracle_mod):
    from heterofusionrcnn_amd import rcnn_data
    _lib, L = abi()
    t = sc.make_inputs(c)
    b, m, g = c["b"], c["m"], c["g"]
    ins = [dev(DEV, t[k]) for k in ("proposals", "proposal_count", "gt", "gt_count")]
    out = torch.full((b, m, max(g, 1)), float("nan"), dtype=torch.float32, device="cuda")
    status = L.hf_box3d_iou_matrix(b, m, g, _lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]) if g else None, _lib.ptr(ins[3]), _lib.ptr(out),
                                   _lib.stream_ptr())
    torch.cuda.synchronize()
    assert status == _lib.HF_OK
    got = host(out)
    if g == 0:
        assert np.isnan(got).all(), "g == 0: the output stays untouched"
        assert tuple(rcnn_data.box3d_iou_matrix(*ins).shape) == (b, m, 0)
        return
    assert not np.isnan(got).any(), "an element was never written"
    want = sc.ref_iou_matrix(c, t)
    assert (got[want == 0] == 0).all(), "padding and disjoint pairs are exactly 0"
    bound, measured = sc.iou_bound(c, t, oracle_mod)
    err = float(np.abs(got.astype(np.float64) - want).max())
    RATIOS["iou"] = max(RATIOS["iou"], err / bound)
    print("IoU matrix of %s: error %.3g, bound %.3g (float32 CPU form %.3g off fp64)" % (sc.case_id(c), err, bound, measured))
    assert err <= bound, "%s: IoU matrix %.3g off fp64, bound %.3g" % (sc.case_id(c), err, bound)
    same_bits(out, rcnn_data.box3d_iou_matrix(*ins), "IoU matrix", c)
