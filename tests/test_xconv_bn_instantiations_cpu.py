"""Kernel set of csrc/xconv_bn.hip, on any machine with hipcc: the file is compiled to assembly with the Makefile's flags and its code
object must hold exactly the three fused kernels with the BatchNorm fold on (the templates of xconv_common.h at GATHER = BN = true) at the
(K, M) their entry points dispatch (the forward also by V2), plus the finalize kernel; none of them may spill a vector register or touch
scratch.  Only the kernel-metadata table is read (names, LDS, registers, spills, scratch).  Run as a script, the module prints the table
committed as profiles/xconv_bn_instantiations.md."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_asm import compile_to_assembly, kernel_table  # noqa: E402
from xconv_runs import check_argument_limits  # noqa: E402

XBN_DISPATCH = ((8, 1), (8, 2), (8, 4))        # HF_XBN_DISPATCH of csrc/xconv_bn.hip = _XBN_KM of pointcnn.py


def expected():
    want = {("xconv_bn_finalize_kernel", ())}
    for k, m in XBN_DISPATCH:
        want |= {("xconv_dw_fwd_kernel", (k, m, True, False, True)), ("xconv_dw_fwd_kernel", (k, m, True, True, True)),
                 ("xconv_dw_bwd_fw_kernel", (k, m, True, True)), ("xconv_bn_bwd_x_kernel", (k, m))}
    return want


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return kernel_table(compile_to_assembly(tmp_path_factory.mktemp("xconv_bn_asm"), "xconv_bn.hip"))


def test_the_kernel_set_is_the_three_twins_at_the_dispatched_arguments_plus_the_finalize(table):
    compiled = {(name, args) for name, args, _ in table}
    assert compiled == expected(), sorted(compiled ^ expected())
    assert len(table) == len(compiled) == 4 * len(XBN_DISPATCH) + 1


def test_the_routing_table_of_the_package_is_the_dispatched_set():
    from heterofusionrcnn_amd import pointcnn
    assert pointcnn._XBN_KM == set(XBN_DISPATCH) and pointcnn._XBN_KM <= pointcnn._XDW_KM


def test_no_kernel_spills_or_uses_scratch(table):
    for name, args, f in table:
        assert f["spill"] == 0 and f["scratch"] == 0, (name, args, f)


def test_the_backward_keeps_four_waves_per_simd(table):
    """xdw_bwd_grid launches four blocks per CU, one wave of each per SIMD: 512 VGPRs / 4 = 128 is what the attribute on
    xconv_dw_bwd_fw_kernel<K, M, true, true> holds the kernel to"""
    seen = 0
    for name, args, f in table:
        if name == "xconv_dw_bwd_fw_kernel":
            seen += 1
            assert args[3] is True and f["vgpr"] <= 128, (args, f["vgpr"])
    assert seen == len(XBN_DISPATCH)


def test_one_past_each_argument_limit_is_refused():
    check_argument_limits()


def render(table):
    lines = ["# Kernels and template instantiations of csrc/xconv_bn.hip", "",
             "Compiled for gfx950 with the Makefile's flags (`-O3 -ffp-contract=off`); produced by",
             "`python tests/test_xconv_bn_instantiations_cpu.py`.  Template arguments: `xconv_dw_fwd_kernel<K, M, GATHER, V2, BN>`,",
             "`xconv_dw_bwd_fw_kernel<K, M, GATHER, BN>`, `xconv_bn_bwd_x_kernel<K, M>`.  LDS is the static part (`xconv_bn_bwd_x_kernel` takes its own at launch).", "",
             "| kernel | template arguments | LDS bytes | VGPRs | spilled VGPRs | spilled SGPRs | scratch bytes |", "|---|---|---:|---:|---:|---:|---:|"]
    for name, args, f in table:
        lines.append("| `%s` | %s | %d | %d | %d | %d | %d |" % (name, ", ".join(str(a).lower() for a in args) or "-", f["lds"], f["vgpr"], f["spill"],
                                                                f["sgpr_spill"], f["scratch"]))
    lines += ["", "%d kernels." % len(table)]
    return "\n".join(lines)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(render(kernel_table(compile_to_assembly(d, "xconv_bn.hip"))))
