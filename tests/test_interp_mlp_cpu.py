"""CPU tests (-m "not gpu") of the feature-propagation first layer on three_nn rows read in place: the built library exports
hf_linear_bn_fwd_interp / hf_linear_wgrad_interp, the binding table lists them, and every documented HF_EINVAL condition is
answered before any device call (dummy host integers stand in for the pointers, as in
test_abi.py::test_c_abi_rejects_bad_arguments_without_a_gpu)."""
import ctypes

import pytest

ONE = ctypes.c_void_p(16)
BIG = 1 << 30


def test_library_exports_the_interp_entry_points():
    from heterofusionrcnn_amd import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hf_linear_bn_fwd_interp", "hf_linear_wgrad_interp"):
        assert hasattr(L, name), "libhfops.so does not export %s" % name
        assert name in _lib.EXPORTED_SYMBOLS


def _fwd(L, rows=1290, c2=36, c1=1, cout=64, points2=ONE, m=64, rows_per_cloud=645, idx=ONE, weight3=ONE, skip=ONE, weight=ONE,
         bias=ONE, z=ONE, running_mean=None, running_var=None, mean=ONE, invstd=ONE, workspace=ONE, workspace_bytes=BIG):
    return L.hf_linear_bn_fwd_interp(rows, c2, c1, cout, points2, m, rows_per_cloud, idx, weight3, skip, weight, bias, z, 1e-3, 0.1,
                                     running_mean, running_var, mean, invstd, workspace, workspace_bytes, None)


def _wgrad(L, rows=1290, cout=64, c2=36, c1=1, grad_z=ONE, points2=ONE, m=64, rows_per_cloud=645, idx=ONE, weight3=ONE, skip=ONE,
           grad_weight=ONE, workspace=ONE, workspace_bytes=BIG):
    return L.hf_linear_wgrad_interp(rows, cout, c2, c1, grad_z, points2, m, rows_per_cloud, idx, weight3, skip, grad_weight, workspace,
                                    workspace_bytes, None)


SHARED_BAD = [dict(rows=0), dict(rows=-5), dict(rows=1291), dict(rows=1 << 32, rows_per_cloud=1 << 31), dict(rows_per_cloud=0),
              dict(m=0), dict(m=-1), dict(c2=0), dict(c2=1025), dict(c1=-1), dict(c1=1025), dict(cout=0), dict(cout=257),
              dict(skip=None), dict(points2=None), dict(idx=None), dict(weight3=None), dict(workspace=None), dict(workspace_bytes=0)]


@pytest.mark.parametrize("bad", SHARED_BAD + [dict(weight=None), dict(z=None), dict(mean=None), dict(invstd=None)], ids=str)
def test_forward_rejects_bad_arguments_without_a_gpu(bad):
    from heterofusionrcnn_amd import _lib
    assert _fwd(_lib.lib(), **bad) == _lib.HF_EINVAL


@pytest.mark.parametrize("bad", SHARED_BAD + [dict(grad_z=None), dict(grad_weight=None)], ids=str)
def test_wgrad_rejects_bad_arguments_without_a_gpu(bad):
    from heterofusionrcnn_amd import _lib
    assert _wgrad(_lib.lib(), **bad) == _lib.HF_EINVAL


def test_workspace_one_byte_short_is_rejected():
    """the sizes are those of the existing queries: hf_linear_bn_fwd_workspace(cout), hf_linear_wgrad_workspace(rows, cout, cin)
    with cin = round_up(c2 + c1, 4)"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    assert _fwd(L, workspace_bytes=L.hf_linear_bn_fwd_workspace(64) - 1) == _lib.HF_EINVAL
    assert _wgrad(L, workspace_bytes=L.hf_linear_wgrad_workspace(1290, 64, 40) - 1) == _lib.HF_EINVAL
    assert _wgrad(L, c2=1024, c1=1024, workspace_bytes=L.hf_linear_wgrad_workspace(1290, 64, 2048) - 1) == _lib.HF_EINVAL
