"""The bf16 inference path without a GPU: the argument contract of the two entry points (HF_EINVAL before any launch), the coverage
guard of tests/linear_bf16_cases.py against the compiled instantiations of csrc/linear_bf16.hip with their resources (read from the
kernel metadata table of the assembly only), and the switch's defaults."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_cases as lc  # noqa: E402
from kernel_asm import LDS_PER_CU, compile_to_assembly, kernel_table  # noqa: E402

# workgroups per CU each instantiation is meant to run with: the 256-thread forms two (amdgpu_waves_per_eu(2)), the 512-thread
# form occupies two waves per SIMD by itself; the LDS must leave room for one more of each, so that a second workgroup can be staged
# while the first drains
INTENDED_WORKGROUPS_PER_CU = {(2, 2): 2, (4, 2): 2, (4, 4): 2}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return kernel_table(compile_to_assembly(tmp_path_factory.mktemp("linear_bf16_asm"), "linear_bf16.hip"))


def test_bad_arguments_return_einval_without_a_gpu():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    ok, off8, off2 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 2)
    E = _lib.HF_EINVAL

    def gemm(rows=8, cin=8, cout=8, x=ok, w=ok, y=ok, bn=(None, None, None, None), mode=0):
        return L.hf_linear_bf16_fwd_eval(rows, cin, cout, x, w, None, *bn, mode, y, None)

    assert gemm(rows=0) == E and gemm(rows=-1) == E
    assert gemm(cin=6) == E and gemm(cin=0) == E and gemm(cout=10) == E and gemm(cout=0) == E
    assert gemm(x=None) == E and gemm(w=None) == E and gemm(y=None) == E
    assert gemm(x=off8) == E and gemm(w=off8) == E and gemm(y=off8) == E
    four = (ok, ok, ok, ok)
    for missing in range(4):                                            # all four or none
        assert gemm(bn=tuple(None if i == missing else ok for i in range(4))) == E
    assert gemm(mode=1) == E and gemm(mode=2) == E and gemm(mode=3) == E  # a mode without the four constants
    assert gemm(bn=four, mode=4) == E and gemm(bn=four, mode=-1) == E
    assert gemm(rows=(1 << 31) * 128, cout=512) == E                    # the grid would not fit 31 bits
    assert L.hf_f32_to_bf16(0, ok, ok, None) == E and L.hf_f32_to_bf16(4, None, ok, None) == E and L.hf_f32_to_bf16(4, ok, None, None) == E
    assert L.hf_f32_to_bf16(4, off2, ok, None) == E


def test_every_compiled_instantiation_is_reached_by_a_case_and_nothing_else(table):
    compiled = {(name, args) for name, args, _ in table}
    selected = lc.selected_instantiations()
    assert not compiled - selected, "compiled but reached by no case: %s" % sorted(compiled - selected)
    assert not selected - compiled, "the dispatch rule restated in linear_bf16_cases.py names kernels that do not exist: %s" % sorted(selected - compiled)
    assert len(table) == len(compiled)
    exact = lc.selected_instantiations(lc.exact_cases())
    assert exact == compiled, "the bit-for-bit family must reach every instantiation on its own"


def test_case_ids_are_unique_and_cover_the_tile_edges():
    cases = lc.all_cases()
    ids = [lc.case_id(c) for c in cases]
    assert len(ids) == len(set(ids))
    rows = {c["rows"] for c in lc.exact_cases()}
    couts = {c["cout"] for c in lc.exact_cases()}
    assert {lc.ROW_TILE - 1, lc.ROW_TILE, lc.ROW_TILE + 1} <= rows
    for tile in lc.COL_TILES:
        assert {tile - 4, tile, tile + 4} <= couts
    assert all(c["cin"] % 4 == 0 and c["cout"] % 4 == 0 for c in cases)
    assert any(c["cin"] % lc.K_STAGE for c in cases) and any(c["cin"] > lc.K_STAGE for c in cases)
    assert all(not lc.MODES[c["mode"]][1] & 2 for c in lc.exact_cases())
    assert {lc.MODES[c["mode"]][1] for c in lc.round_cases()} == {0, 1, 2, 3}


def test_no_spills_no_scratch_and_the_lds_fits(table):
    for name, args, f in table:
        assert f["spill"] == 0 and f["sgpr_spill"] == 0 and f["scratch"] == 0, (name, args, f)
        assert f["vgpr"] <= 256, (name, args, f)
        if name == "linear_bf16_kernel":
            assert f["lds"] * INTENDED_WORKGROUPS_PER_CU[args] <= LDS_PER_CU, (name, args, f["lds"])


def test_precision_switch_defaults_to_fp32_and_restores():
    from heterofusionrcnn_amd import mlp
    assert mlp.inference_precision_name() == "fp32"
    with mlp.inference_precision("bf16"):
        assert mlp.inference_precision_name() == "bf16"
        with mlp.inference_precision("fp32"):
            assert mlp.inference_precision_name() == "fp32"
        assert mlp.inference_precision_name() == "bf16"
    assert mlp.inference_precision_name() == "fp32"
    with pytest.raises(ValueError):
        mlp.inference_precision("fp16")
    import torch
    w = torch.zeros(64, 64)
    with mlp.inference_precision("bf16"), torch.no_grad():
        assert not mlp.bf16_route(torch.zeros(1 << 16, 64), w)          # a host tensor never takes the kernel
    assert not mlp.bf16_route_pays(1 << 20, 28, 512) and not mlp.bf16_route_pays(1 << 20, 6, 256)   # cin < 32 stays fp32


def test_detect_parser_and_detector_accept_precision():
    from heterofusionrcnn_amd import detect
    ap = detect.build_parser()
    assert ap.parse_args(["d", "a.pt", "b.pt", "out"]).precision == "fp32"
    assert ap.parse_args(["d", "a.pt", "b.pt", "out", "--precision", "bf16"]).precision == "bf16"
    with pytest.raises(SystemExit):
        ap.parse_args(["d", "a.pt", "b.pt", "out", "--precision", "fp8"])
    import inspect
    from heterofusionrcnn_amd.two_stage import TwoStageDetector
    assert inspect.signature(detect.detect).parameters["precision"].default == "fp32"
    assert inspect.signature(TwoStageDetector.__init__).parameters["precision"].default == "fp32"
