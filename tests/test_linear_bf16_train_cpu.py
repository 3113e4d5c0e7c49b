"""The bf16 training path without a GPU: the argument contract of the new entry points (HF_EINVAL before any launch), the coverage guard
of tests/linear_bf16_train_cases.py against the compiled instantiations of csrc/linear_bf16_train.hip with their resources (read from
the kernel metadata table of the assembly only), the training-precision switch, the parsers and the checkpoint settings."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_train_cases as tc  # noqa: E402
from kernel_asm import LDS_PER_CU, compile_to_assembly, kernel_table  # noqa: E402

# workgroups per CU each instantiation is meant to run with under amdgpu_waves_per_eu(2): the 256-thread form (one wave per SIMD) two,
# the 512-thread form (two waves per SIMD) one
INTENDED_WORKGROUPS_PER_CU = {(2,): 2, (4,): 1}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return kernel_table(compile_to_assembly(tmp_path_factory.mktemp("linear_bf16_train_asm"), "linear_bf16_train.hip"))


def test_bad_arguments_return_einval_without_a_gpu():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    ok, off8, off2, off1 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 2), ctypes.c_void_p(4096 + 1)
    E = _lib.HF_EINVAL
    need = L.hf_linear_bf16_wgrad_workspace(1000, 64, 64)
    assert need == 4 * tc.plan(1000, 64, 64)[2] * 64 * 64

    def wg(rows=1000, cout=64, cin=64, g=ok, x=ok, dw=ok, ws=ok, nbytes=need):
        return L.hf_linear_bf16_wgrad(rows, cout, cin, g, x, dw, ws, nbytes, None)

    assert wg(rows=0) == E and wg(rows=-1) == E
    assert wg(cout=6) == E and wg(cout=0) == E and wg(cin=10) == E and wg(cin=0) == E and wg(cout=32772) == E and wg(cin=32772) == E
    assert wg(g=None) == E and wg(x=None) == E and wg(dw=None) == E
    assert wg(g=off8) == E and wg(x=off8) == E and wg(dw=off8) == E and wg(ws=off8) == E
    assert wg(ws=None) == E and wg(nbytes=need - 1) == E and wg(nbytes=0) == E          # a missing or short workspace
    assert L.hf_linear_bf16_wgrad_workspace(0, 64, 64) == 0 and L.hf_linear_bf16_wgrad_workspace(8, 6, 64) == 0

    def tr(rows=8, cols=8, src=ok, dst=ok):
        return L.hf_f32_to_bf16_transpose(rows, cols, src, dst, None)

    assert tr(rows=0) == E and tr(cols=0) == E and tr(rows=-4) == E and tr(src=None) == E and tr(dst=None) == E
    assert tr(src=off2) == E and tr(dst=off1) == E
    assert tr(rows=1 << 30, cols=1 << 30) == E                                          # the grid would not fit 31 bits


@pytest.mark.parametrize("rows,cout,cin", [(c["rows"], c["cout"], c["cin"]) for c in tc.all_cases()[::5]] + [(131072, 256, 320), (409600, 512, 2688)])
def test_the_restated_plan_is_the_librarys(rows, cout, cin):
    from heterofusionrcnn_amd import _lib
    assert _lib.lib().hf_linear_bf16_wgrad_workspace(rows, cout, cin) == 4 * tc.plan(rows, cout, cin)[2] * cout * cin


def test_every_compiled_instantiation_is_reached_by_a_case_and_nothing_else(table):
    compiled = {(name, args) for name, args, _ in table}
    selected = tc.selected_instantiations()
    assert not compiled - selected, "compiled but reached by no case: %s" % sorted(compiled - selected)
    assert not selected - compiled, "the dispatch rule restated in linear_bf16_train_cases.py names kernels that do not exist: %s" % sorted(selected - compiled)
    assert len(table) == len(compiled)
    assert tc.selected_instantiations(tc.exact_cases()) == compiled, "the bit-for-bit family must reach every instantiation on its own"


def test_case_ids_are_unique_and_cover_the_edges():
    cases = tc.all_cases()
    ids = [tc.case_id(c) for c in cases]
    assert len(ids) == len(set(ids))
    exact = tc.exact_cases()
    rows = {c["rows"] for c in exact}
    assert {1, tc.K_STEP - 1, tc.K_STEP, tc.K_STEP + 1, tc.STAGE - 1, tc.STAGE, tc.STAGE + 1, tc.MIN_CHUNK - 1, tc.MIN_CHUNK, tc.MIN_CHUNK + 1} <= rows
    assert all(64 * c["rows"] < 2 ** 24 for c in exact)
    couts, cins = {c["cout"] for c in exact}, {c["cin"] for c in exact}
    assert 4 in couts and 4 in cins and {tc.OUT_TILE - 4, tc.OUT_TILE, tc.OUT_TILE + 4} <= couts
    for tile in tc.IN_TILES:
        assert {tile - 4, tile, tile + 4} <= cins
    assert all(c["cin"] % 4 == 0 and c["cout"] % 4 == 0 for c in cases)
    chunks = [tc.plan(c["rows"], c["cout"], c["cin"])[2] for c in exact]
    assert 1 in chunks and 2 in chunks and max(chunks) >= tc.REDUCE_UNROLLED_FROM
    assert any(tc.REDUCE_UNROLLED_FROM <= n and n % 64 for n in chunks)               # the unrolled loop of the reduction and its tail
    assert max(tc.workgroups(c["rows"], c["cout"], c["cin"]) for c in exact) > tc.CU_RESIDENT_WORKGROUPS
    rnd = tc.round_cases()
    assert len(rnd) == 3 and all(200 <= c["rows"] <= 5000 for c in rnd)
    assert any(c["cin"] > max(tc.IN_TILES) for c in rnd) and any(c["cout"] > tc.OUT_TILE for c in rnd)
    shapes = tc.transpose_cases()
    assert (4, 4) in shapes and any(r == 1 for r, _ in shapes) and any(r % tc.TR_TILE == 0 and c % tc.TR_TILE == 0 for r, c in shapes)
    assert any(r % tc.TR_TILE and c % tc.TR_TILE for r, c in shapes)


def test_no_spills_no_scratch_and_the_lds_fits(table):
    for name, args, f in table:
        assert f["spill"] == 0 and f["sgpr_spill"] == 0 and f["scratch"] == 0, (name, args, f)
        assert f["vgpr"] <= 256, (name, args, f)
        if name == "wgrad_bf16_kernel":
            assert f["lds"] * INTENDED_WORKGROUPS_PER_CU[args] <= LDS_PER_CU, (name, args, f["lds"])


def test_training_precision_defaults_to_fp32_nests_and_restores():
    from heterofusionrcnn_amd import mlp
    assert mlp.training_precision_name() == "fp32"
    with mlp.training_precision("bf16"):
        assert mlp.training_precision_name() == "bf16"
        with mlp.training_precision("fp32"):
            assert mlp.training_precision_name() == "fp32"
        assert mlp.training_precision_name() == "bf16"
    assert mlp.training_precision_name() == "fp32"
    with pytest.raises(ValueError):
        mlp.training_precision("fp16")
    with pytest.raises(RuntimeError):
        with mlp.training_precision("bf16"):
            raise RuntimeError("leaves the block")
    assert mlp.training_precision_name() == "fp32"


def test_the_two_switches_are_separate():
    import torch
    from heterofusionrcnn_amd import mlp
    with mlp.inference_precision("bf16"):
        assert mlp.training_precision_name() == "fp32"
        assert not mlp.bf16_train_route(torch.zeros(1 << 16, 64), torch.zeros(64, 64))
    with mlp.training_precision("bf16"):
        assert mlp.inference_precision_name() == "fp32"
        assert not mlp.bf16_train_route(torch.zeros(1 << 16, 64), torch.zeros(64, 64))       # a host tensor never takes the kernels
        with torch.no_grad():
            assert not mlp.bf16_route(torch.zeros(1 << 16, 64), torch.zeros(64, 64))
    assert not mlp.bf16_train_route_pays(1 << 20, 28, 512) and not mlp.bf16_train_route_pays(1 << 20, 6, 256)   # cin < 32 stays fp32
    assert isinstance(mlp.BF16_TRAIN_ROUTED_CALLS[0], int)


def test_train_parsers_accept_precision():
    import inspect
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    for ap, argv in ((train_rpn.build_parser(), ["data"]), (train_rcnn.build_parser(), ["data", "handoff"])):
        assert ap.parse_args(argv).precision == "fp32"
        assert ap.parse_args(argv + ["--precision", "bf16"]).precision == "bf16"
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ["--precision", "fp8"])
    assert inspect.signature(train_rpn.train).parameters["precision"].default == "fp32"
    assert inspect.signature(train_rcnn.train).parameters["precision"].default == "fp32"


def test_checkpoint_settings_record_the_precision_only_when_it_is_not_fp32(tmp_path):
    from heterofusionrcnn_amd import checkpoint as C
    plain = C.train_op_settings(1e-3, None, 0.0, False)
    assert "precision" not in plain and C.train_op_settings(1e-3, None, 0.0, False, "fp32") == plain
    bf16 = C.train_op_settings(1e-3, None, 0.0, False, "bf16")
    assert bf16["precision"] == "bf16" and {k: v for k, v in bf16.items() if k != "precision"} == plain
    for written, other in ((bf16, plain), (plain, bf16)):
        ck = {"config": "rpn_multiclass", "settings": written}
        C.check_resumable(ck, "rpn_multiclass", written, "ckpt")
        with pytest.raises(ValueError):
            C.check_resumable(ck, "rpn_multiclass", other, "ckpt")
