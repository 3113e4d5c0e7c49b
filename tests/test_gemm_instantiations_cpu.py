"""Coverage guard of the GEMM parity suite, on any machine with hipcc: csrc/gemm.hip is compiled to assembly with the Makefile's
flags, and the set of kernels in the code object must equal the set of template instantiations that the cases of
tests/gemm_cases.py select by the documented dispatch rule.  A new instantiation cannot land without a case, and a case table that
stops reaching an instantiation fails here without a GPU.  Run as a script, the module prints the resource table committed as
profiles/gemm_instantiations.md."""
import os
import re
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402
from kernel_asm import CSRC, LDS_PER_CU, compile_to_assembly, demangle, kernel_table  # noqa: E402


def kernels_with_two_waves_per_eu():
    """the kernels of gemm.hip that carry amdgpu_waves_per_eu(2): two workgroups of four waves share a CU and its LDS"""
    with open(os.path.join(CSRC, "gemm.hip")) as f:
        return set(re.findall(r"amdgpu_waves_per_eu\(2\)\)\)\s*void\s+(\w+)\s*\(", f.read()))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return kernel_table(compile_to_assembly(tmp_path_factory.mktemp("gemm_asm")))


def test_demangle_reads_template_arguments():
    assert demangle("_ZN2hf12wgrad_kernelILi2ELi2ELb1ELb0EEEvxiiixPKfS2_S2_S2_S2_S2_PfNS_9GatherSrcE") == ("wgrad_kernel", (2, 2, True, False))
    assert demangle("_ZN2hf19wgrad_reduce_kernelEiiPKfPf") == ("wgrad_reduce_kernel", ())


def test_case_ids_are_unique():
    ids = [gc.case_id(c) for c in gc.all_cases()]
    assert len(ids) == len(set(ids))


def test_every_compiled_instantiation_is_selected_by_a_case_and_nothing_else(table):
    compiled = {(name, args) for name, args, _ in table}
    selected = gc.selected_instantiations()
    assert not compiled - selected, "compiled but reached by no case of gemm_cases.py: %s" % sorted(compiled - selected)
    assert not selected - compiled, "the dispatch rule restated in gemm_cases.py names kernels that do not exist: %s" % sorted(selected - compiled)
    assert len(table) == len(compiled)


def test_exact_family_alone_reaches_every_gemm_instantiation(table):
    """the bit-for-bit family is the one that sees dropped rows and stale prefetches: it must not depend on the rounding family for
    its reach (the training pair of the lifting chain is rounding-family only: its batch statistics are not integers)"""
    compiled = {(name, args) for name, args, _ in table}
    exact = gc.selected_instantiations([c for c in gc.all_cases() if c["family"] == "exact"])
    rounding_only = {name for name, _ in compiled - exact}
    assert rounding_only <= {"lift_stats_kernel", "lift_linear_bwd_kernel", "lift_wgrad_kernel"}, sorted(compiled - exact)


def test_two_workgroups_fit_a_compute_unit(table):
    two_per_cu = kernels_with_two_waves_per_eu()
    assert len(two_per_cu) >= 4 and two_per_cu <= {name for name, _, _ in table}
    for name, args, f in table:
        assert f["vgpr"] <= 256, (name, args)
        if name in two_per_cu:
            assert f["lds"] <= LDS_PER_CU // 2, (name, args, f["lds"])


def render(table, source="gemm.hip"):
    if source == "gemm.hip":
        lines = ["# Template instantiations of csrc/gemm.hip", "",
                 "Compiled for gfx950 with the Makefile's flags (`-O3 -ffp-contract=off`); produced by",
                 "`python tests/test_gemm_instantiations_cpu.py`.  NT >= 5 spills: the evidence behind the routing thresholds",
                 "`FUSED_FWD_MAX_COUT = 224` and `cin <= 160` of `heterofusionrcnn_amd/mlp.py`.", ""]
    else:
        lines = ["## csrc/%s" % source, ""]
    lines += ["| kernel | template arguments | LDS bytes | VGPRs | spilled VGPRs | scratch bytes |", "|---|---|---:|---:|---:|---:|"]
    for name, args, f in table:
        lines.append("| `%s` | %s | %d | %d | %d | %d |" % (name, ", ".join(str(a).lower() for a in args) or "-", f["lds"], f["vgpr"],
                                                           f["spill"], f["scratch"]))
    lines += ["", "%d kernels." % len(table)]
    return "\n".join(lines)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(render(kernel_table(compile_to_assembly(d))))
        print()
        print(render(kernel_table(compile_to_assembly(d, "fp_linear.hip")), "fp_linear.hip"))
