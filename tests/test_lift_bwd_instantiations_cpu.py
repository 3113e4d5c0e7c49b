"""Resource guard of csrc/lift_bwd.hip, on any machine with hipcc: the file is compiled to assembly with the Makefile's flags; no
kernel may spill a register or use scratch, two workgroups of the sweep must fit a compute unit, and the compiled set must equal the
instantiations that the shapes of tests/lift_bwd_cases.py (run by test_lift_bwd_onepass_abi.py) select.  The table is the evidence for the file's choice to sum
B_d and C_d in the sweep's epilogue and for the entry's limit c0 <= 128.  Run as a script, the module prints
profiles/lift_bwd_instantiations.md."""
import os
import re
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_asm as ka  # noqa: E402
import lift_bwd_cases as lb  # noqa: E402

SOURCE = "lift_bwd.hip"


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return ka.kernel_table(ka.compile_to_assembly(tmp_path_factory.mktemp("lift_bwd_asm"), SOURCE))


def kernels_with_two_waves_per_eu():
    with open(os.path.join(ka.CSRC, SOURCE)) as f:
        return set(re.findall(r"amdgpu_waves_per_eu\(2\)\)\)\s*void\s+(\w+)\s*\(", f.read()))


def test_nothing_spills_and_nothing_uses_scratch(table):
    for name, args, f in table:
        assert f["spill"] == 0 and f["sgpr_spill"] == 0 and f["scratch"] == 0, (name, args, f)


def test_two_workgroups_fit_a_compute_unit(table):
    two_per_cu = kernels_with_two_waves_per_eu()
    assert two_per_cu == {"lift_bwd_onepass_kernel"}
    for name, args, f in table:
        assert f["vgpr"] <= 256, (name, args)
        if name in two_per_cu:
            assert f["lds"] <= 80 * 1024 == ka.LDS_PER_CU // 2, (name, args, f["lds"])


def test_the_compiled_set_is_what_the_abi_tests_shapes_select(table):
    compiled = {(name, args) for name, args, _ in table}
    selected = lb.selected_instantiations()
    assert compiled == selected, (sorted(compiled - selected), sorted(selected - compiled))
    assert len(table) == len(compiled)
    assert {args[0] for name, args in compiled if name == "lift_bwd_onepass_kernel"} == set(range(1, lb.MAX_C0 // 32 + 1))


def render(table):
    lines = ["# Kernels and template instantiations of csrc/lift_bwd.hip", "",
             "Compiled for gfx950 with the Makefile's flags (`-O3 -ffp-contract=off`); produced by",
             "`python tests/test_lift_bwd_instantiations_cpu.py`.  `lift_bwd_onepass_kernel<NT, VEC>` keeps eleven sums per lane and column;",
             "it carries `amdgpu_waves_per_eu(2)`, so 256 VGPRs and 80 KB of LDS are its limits.", "",
             "| kernel | template arguments | LDS bytes | VGPRs | spilled VGPRs | spilled SGPRs | scratch bytes |", "|---|---|---:|---:|---:|---:|---:|"]
    for name, args, f in table:
        lines.append("| `%s` | %s | %d | %d | %d | %d | %d |" % (name, ", ".join(str(a).lower() for a in args) or "-", f["lds"], f["vgpr"],
                                                                f["spill"], f["sgpr_spill"], f["scratch"]))
    lines += ["", "%d kernels." % len(table)]
    return "\n".join(lines)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(render(ka.kernel_table(ka.compile_to_assembly(d, SOURCE))))
