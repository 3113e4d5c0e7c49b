"""CPU tests (-m "not gpu"): the C-ABI library loads and exports every symbol include/hfops.h
declares; the Python host layer validates arguments like the reference's OP_REQUIRES and has
no CPU fallback.  No compute call is made here (there is no GPU in this container)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "hfops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(hf_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from heterofusionrcnn_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 24
    for n in names:
        assert hasattr(L, n), "libhfops.so does not export %s" % n
    # and the binding table covers exactly the header
    assert sorted(_lib.EXPORTED_SYMBOLS) == names


def test_version_and_strerror():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    assert b"gfx950" in L.hf_version()
    assert L.hf_strerror(0) == b"ok"
    assert b"invalid" in L.hf_strerror(-1)
    assert L.hf_fps_onchip_limit() == 16384
    assert L.hf_fps_workspace(8, 16384) == 0 and L.hf_fps_workspace(2, 20000) == 2 * 20000 * 4
    pad = lambda b: (b + 255) & ~255
    # dense mask + per-column-block counters + per-column-block lists (2048 x 16 bytes) + transposed diagonal words
    # + the per-box table (80 bytes per box) + the words next to the diagonal
    assert L.hf_oriented_nms_workspace(9000) == pad(9000 * 141 * 8) + pad(141 * 4) + 141 * 2048 * 16 + pad(9000 * 8) + pad(9000 * 80) + pad(9000 * 8)


def test_no_cpu_fallback():
    import heterofusionrcnn_amd as hf
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        hf.query_ball_point(0.1, 4, torch.zeros(1, 4, 3), torch.zeros(1, 2, 3))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        hf.farthest_point_sample(2, torch.zeros(1, 4, 3))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        hf.compute_bev_iou(torch.zeros(1, 5), torch.zeros(1, 5))


def test_argument_checks_mirror_op_requires():
    """same conditions as the OP_REQUIRES lines (tf_grouping.cpp:70-85, tf_sampling.cpp:100-106,
    bev_iou.cpp:52,65,156-157, tf_cropping.cpp:108-125); raised before any device work"""
    import heterofusionrcnn_amd as hf
    x = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match="positive radius"):
        hf.query_ball_point(0.0, 4, x, x)
    with pytest.raises(ValueError, match="positive nsample"):
        hf.query_ball_point(0.1, 0, x, x)
    with pytest.raises(ValueError, match="xyz1 shape"):
        hf.query_ball_point(0.1, 4, torch.zeros(1, 4, 2), x)
    with pytest.raises(ValueError, match="positive npoint"):
        hf.farthest_point_sample(0, x)
    with pytest.raises(ValueError, match="inp shape"):
        hf.gather_point(torch.zeros(1, 4, 4), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="idx shape"):
        hf.group_point(torch.zeros(2, 4, 3), torch.zeros(1, 2, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="proposals shape"):
        hf.compute_bev_iou(torch.zeros(0, 5), torch.zeros(1, 5))
    with pytest.raises(ValueError, match="nms_threshold"):
        hf.oriented_nms(torch.zeros(3, 5), -0.1)
    with pytest.raises(ValueError, match="positive resize"):
        hf.pc_crop_and_sample(x, x, torch.zeros(1, 4, 1), torch.zeros(1, 4, dtype=torch.bool), torch.zeros(1, 3, 8),
                              torch.zeros(1, dtype=torch.int32), 0)
    with pytest.raises(NotImplementedError):
        hf.prob_sample(None, None)
    # no silent framework path: shapes the HIP kNN kernels do not cover raise unless the caller asks for the dense form
    with pytest.raises(ValueError, match="dense=True"):
        hf.knn_point(2, torch.zeros(1, 8, 4), torch.zeros(1, 3, 4))
    with pytest.raises(ValueError, match="dense=True"):
        hf.knn_point(68, torch.zeros(1, 80, 3), torch.zeros(1, 3, 3))
    val, idx = hf.knn_point(2, torch.arange(32.).reshape(1, 8, 4), torch.zeros(1, 3, 4), dense=True)
    assert idx.tolist() == [[[0, 1]] * 3] and val.shape == (1, 3, 2)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    """HF_EINVAL paths return before any HIP call, so they are testable on the CPU box"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    assert L.hf_query_ball_point(1, 4, 2, -1.0, 4, one, one, one, one, None) == _lib.HF_EINVAL
    assert L.hf_query_ball_point(1, 4, 2, 0.1, 0, one, one, one, one, None) == _lib.HF_EINVAL
    assert L.hf_query_ball_point(1, 4, 2, float("nan"), 4, one, one, one, one, None) == _lib.HF_EINVAL
    assert L.hf_farthest_point_sample(1, 4, 0, one, None, one, None) == _lib.HF_EINVAL
    assert L.hf_farthest_point_sample(1, 20000, 8, one, None, one, None) == _lib.HF_EWORKSPACE
    assert L.hf_compute_bev_iou(0, one, 1, one, one, one, None) == _lib.HF_EINVAL
    assert L.hf_oriented_nms(one, 8, -1.0, one, None, one, 1 << 20, None) == _lib.HF_EINVAL
    assert L.hf_oriented_nms(one, 8, 0.5, one, None, None, 0, None) == _lib.HF_EWORKSPACE
    assert L.hf_pc_crop_and_sample(one, one, one, one, one, one, 1, 1, 4, 0, 1, 1, one, one, one, one, one, one,
                                   None) == _lib.HF_EINVAL
    # empty problems are OK and launch nothing
    assert L.hf_query_ball_point(0, 4, 2, 0.1, 4, one, one, one, one, None) == _lib.HF_OK
    assert L.hf_group_point(0, 4, 3, 2, 2, one, one, one, None) == _lib.HF_OK


def test_loss_entry_points_reject_bad_arguments_without_a_gpu():
    """hf_rpn_loss_fwd / _bwd and hf_rcnn_loss_fwd / _bwd: the limits of the register arrays (k + 1 <= 8, bins in 1..32), every NULL
    input one at a time, NULL outputs, and the workspace: all of it returns before any HIP call (fake non-null pointers, never
    dereferenced).  No call below has a full set of valid arguments"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(256)
    EINVAL, EWS = _lib.HF_EINVAL, _lib.HF_EWORKSPACE
    for kind, n_in, floats in (("rpn", 11, (100.0, 1.0, 1.0)), ("rcnn", 13, (0.45, 0.6, 0.55, 1.0, 1.0))):
        need = getattr(L, "hf_%s_loss_workspace" % kind)()
        assert need == 4 * (4 if kind == "rpn" else 5) * 1024
        fwd_fn, bwd_fn = getattr(L, "hf_%s_loss_fwd" % kind), getattr(L, "hf_%s_loss_bwd" % kind)

        def fwd(rows=10, k=3, nbx=12, nbt=12, null=None, out=one, ws=one, nbytes=need):
            ins = [None if i == null else one for i in range(n_in)]
            return fwd_fn(rows, k, nbx, nbt, *ins, *floats, out, ws, nbytes, None)

        def bwd(rows=10, k=3, nbx=12, nbt=12, null=None, out=one, up=one, g_logits=one, g_head=one):
            ins = [None if i == null else one for i in range(n_in)]
            return bwd_fn(rows, k, nbx, nbt, *ins, *floats, out, up, g_logits, g_head, None)

        bad = {}
        for name, f in (("fwd", fwd), ("bwd", bwd)):
            bad.update({"%s: rows < 0" % name: f(rows=-1), "%s: k = 0" % name: f(k=0), "%s: k = 8" % name: f(k=8), "%s: nbx = 0" % name: f(nbx=0),
                        "%s: nbx = 33" % name: f(nbx=33), "%s: nbt = 33" % name: f(nbt=33), "%s: nbt = 0" % name: f(nbt=0), "%s: no out" % name: f(out=None)})
            bad.update({"%s: input %d is NULL" % (name, i): f(null=i) for i in range(n_in)})
        bad.update({"bwd: no upstream": bwd(up=None), "bwd: no logit gradient": bwd(g_logits=None), "bwd: no grad_head": bwd(g_head=None),
                    "fwd: rows = 0, no out": fwd(rows=0, out=None), "bwd: rows = 0, no upstream": bwd(rows=0, up=None)})
        wrong = {name: got for name, got in bad.items() if got != EINVAL}
        assert not wrong, (kind, wrong)
        assert fwd(ws=None) == EWS and fwd(nbytes=need - 1) == EWS and fwd(nbytes=0) == EWS and fwd(rows=0, ws=None) == EWS
        # the limits themselves pass the argument check: with them only the workspace is left to refuse
        assert fwd(k=7, nbx=32, nbt=32, ws=None) == EWS and fwd(k=1, nbx=1, nbt=1, nbytes=need - 1) == EWS
        assert bwd(rows=0) == _lib.HF_OK and bwd(rows=0, g_logits=None, g_head=None) == _lib.HF_OK       # empty: nothing is launched


def test_product_library_reads_no_environment_variable():
    """the diagnostic knobs of the kernels (phase exits that leave outputs unwritten, forced tile shapes, kernel overrides) exist
    only in -DHF_DIAG builds: the shipped library neither imports getenv nor carries their names"""
    import subprocess
    from heterofusionrcnn_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    for name in (b"HF_QBP_", b"HF_BEV_STOP", b"HF_NMS_STOP", b"HF_GEMM_ROUNDS", b"HF_BALL_QUERY", b"HF_FPS"):
        assert name not in blob, name
    syms = subprocess.run(["nm", "-D", "--undefined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "getenv" not in syms


def test_ball_query_variant_and_workspace_argument_checks():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    assert L.hf_ball_query_workspace(0, 100) == 0
    # per cloud: 16 bytes per point + the bucket table (1024 / 4096 / 16384 buckets + 4 words), 16-byte multiples
    assert L.hf_ball_query_workspace(2, 1000) == 2 * (16 * 1000 + 4 * (1024 + 4))
    assert L.hf_ball_query_workspace(8, 16384) == 8 * (16 * 16384 + 4 * (16384 + 4))
    args = (1, 64, 8, 0.5, 4, one, one, 1, one, one, one)
    assert L.hf_query_ball_group_xyz_ws(7, *args, None, 0, None) == _lib.HF_EINVAL                # unknown variant
    assert L.hf_query_ball_group_xyz_ws(3, *args, None, 0, None) == _lib.HF_EWORKSPACE            # sorted needs a workspace
    assert L.hf_query_ball_group_xyz_ws(3, *args, one, 16, None) == _lib.HF_EWORKSPACE            # ... of the right size
    assert L.hf_query_ball_group_xyz_ws(0, 1, 64, 8, -1.0, 4, one, one, 1, one, one, one, None, 0, None) == _lib.HF_EINVAL
    assert L.hf_farthest_point_sample_variant(5, 0, 1, 64, 8, one, None, one, None) == _lib.HF_EINVAL
    assert L.hf_farthest_point_sample_variant(1, 300, 1, 64, 8, one, None, one, None) == _lib.HF_EINVAL
    assert L.hf_farthest_point_sample_variant(1, 256, 1, 8000, 8, one, None, one, None) == _lib.HF_EINVAL


def test_xconv_gather_and_elu_chain_argument_checks():
    """round-3 entry points: the in-place feature read of the X-Conv and the ELU-order MFMA layers"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    ok = (2, 100, 50, 8, 64, 32, 1)                                   # b, n_src, rows_per_cloud, k, c0, c1, m
    assert L.hf_xconv_depthwise_gather(2, 100, 50, 8, 48, 32, 1, one, one, one, one, one, one, None) == _lib.HF_EINVAL     # c0 % 64
    assert L.hf_xconv_depthwise_gather(2, 100, 50, 8, 64, 0, 1, one, one, one, one, one, one, None) == _lib.HF_EINVAL      # nothing to gather
    assert L.hf_xconv_depthwise_gather(*ok, one, one, None, one, one, one, None) == _lib.HF_EINVAL                          # no feature table
    assert L.hf_xconv_depthwise_gather(0, 100, 50, 8, 64, 32, 1, one, one, one, one, one, one, None) == _lib.HF_OK          # empty batch
    # [gradient of the gathered block, 256-byte multiple][one row of k * (c0 + c1) * m partial weight sums per row chunk]
    ws = L.hf_xconv_depthwise_gather_grad_workspace(2, 50, 8, 64, 32, 1)
    gathered = (4 * 2 * 50 * 8 * 32 + 255) // 256 * 256
    assert ws > gathered and (ws - gathered) % (4 * 8 * 96) == 0
    assert L.hf_xconv_depthwise_gather_grad_workspace(0, 50, 8, 64, 32, 1) == 0
    grads_none = (None, None, None, None)
    assert L.hf_xconv_depthwise_gather_grad(*ok, one, one, one, one, one, one, one, one, *grads_none, None, 0, None) == _lib.HF_EINVAL
    # a gradient of the feature table needs the inverse neighbour table; a workspace must be large enough
    assert L.hf_xconv_depthwise_gather_grad(*ok, one, one, one, one, one, one, None, None, None, None, one, None, None, 0,
                                            None) == _lib.HF_EINVAL
    assert L.hf_xconv_depthwise_gather_grad(*ok, one, one, one, one, one, one, one, one, None, None, one, None, one, 64,
                                            None) == _lib.HF_EWORKSPACE
    # ELU-order input gradient: the layer below is what it exists for
    assert L.hf_linear_elu_bn_bwd(1024, 64, 64, one, one, one, None, one, one, one, one, one, one, one, 1 << 20, None) == _lib.HF_EINVAL
    assert L.hf_linear_elu_bn_fwd(1024, 3, 512, one, None, None, None, None, None, one, one, 1e-3, 0.01, None, None, one, one, one, 1 << 20,
                                  None) == _lib.HF_EINVAL                                                                       # cout <= 256


def test_bn_dropout_and_narrow_linear_argument_checks():
    """round-4 entry points: dropout fused into the BatchNorm passes, the input gradient of the narrow (segmentation) head"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    big = 1 << 24
    fwd = lambda rate, state=one, seed=one, wsb=big: L.hf_bn_dropout_fwd_train(4096, 64, one, one, one, 1e-3, 0.01, None, None, 2, rate, 0, state,
                                                                               seed, one, one, one, one, wsb, None)
    assert fwd(1.0) == _lib.HF_EINVAL and fwd(-0.1) == _lib.HF_EINVAL and fwd(float("nan")) == _lib.HF_EINVAL      # 0 <= rate < 1
    assert fwd(0.5, state=None) == _lib.HF_EINVAL and fwd(0.5, seed=None) == _lib.HF_EINVAL                       # the layer's state / the call's seed
    assert fwd(0.5, wsb=16) == _lib.HF_EWORKSPACE
    bwd = lambda rate, seed=one, wsb=big: L.hf_bn_dropout_bwd(4096, 64, one, one, one, one, one, one, 2, rate, seed, one, one, one, one, wsb, None)
    assert bwd(1.0) == _lib.HF_EINVAL and bwd(0.5, seed=None) == _lib.HF_EINVAL and bwd(0.5, wsb=16) == _lib.HF_EWORKSPACE
    assert L.hf_narrow_linear_dx(4096, 256, 5, one, one, one, None) == _lib.HF_EINVAL                               # at most four outputs
    assert L.hf_narrow_linear_dx(4096, 256, 2, one, None, one, None) == _lib.HF_EINVAL
    assert L.hf_narrow_linear_dx(0, 256, 2, one, one, one, None) == _lib.HF_EINVAL
    # inference lifting chain with the second layer's constants: all four of them, and the workspace of the training form
    args = (4096, 64, 64, one, one, one, one, one, one, one)
    assert L.hf_lift_elu_fwd_eval_bn(*args, one, one, one, None, one, one, big, None) == _lib.HF_EINVAL
    assert L.hf_lift_elu_fwd_eval_bn(*args, one, one, one, one, one, one, 16, None) == _lib.HF_EWORKSPACE
