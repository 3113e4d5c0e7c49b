"""Coverage guard of the image pyramid's parity suites, on any machine with hipcc: csrc/conv_nhwc.hip is compiled to assembly with the
Makefile's flags, and the set of kernels in the code object must equal the set of template instantiations that the C-ABI cases of
tests/image_pyramid_cases.py and tests/image_pyramid_train_cases.py select by the restated dispatch rules.  A new instantiation cannot
land without a case, and a case table that stops reaching an instantiation fails here without a GPU.  Only kernel names and the
resource fields of the metadata are read.  Run as a script, the module prints the resource table committed as
profiles/conv_nhwc_instantiations.md."""
import os
import re
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_pyramid_cases as pc  # noqa: E402
import image_pyramid_train_cases as tc  # noqa: E402
from kernel_asm import CSRC, LDS_PER_CU, compile_to_assembly, kernel_table  # noqa: E402

SOURCE = "conv_nhwc.hip"
GEMM_FORM = ("conv3x3_kernel", "conv_wgrad_kernel")


def all_cases():
    return pc.abi_cases() + tc.abi_cases()


def kernels_with_two_waves_per_eu():
    """the kernels of conv_nhwc.hip that carry amdgpu_waves_per_eu(2): two workgroups of four waves share a CU and its LDS"""
    with open(os.path.join(CSRC, SOURCE)) as f:
        return set(re.findall(r"amdgpu_waves_per_eu\(2\)\)\)\s*void\s+(\w+)\s*\(", f.read()))


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return kernel_table(compile_to_assembly(tmp_path_factory.mktemp("conv_nhwc_asm"), SOURCE))


def test_case_ids_are_unique():
    ids = [c["id"] for c in all_cases()]
    assert len(ids) == len(set(ids))
    assert {c["family"] for c in all_cases()} == {"round", "exact", "regime"}


def test_every_compiled_instantiation_is_selected_by_a_case_and_nothing_else(table):
    compiled = {(name, args) for name, args, _ in table}
    selected = tc.selected_instantiations()
    assert not compiled - selected, "compiled but reached by no case: %s" % sorted(compiled - selected)
    assert not selected - compiled, "the restated dispatch rules name kernels that do not exist: %s" % sorted(selected - compiled)
    assert len(table) == len(compiled) == 44


def test_exact_family_alone_reaches_every_gemm_form_instantiation(table):
    """the bit-for-bit family is the one that sees a dropped product or a stale prefetch at any summation order: its reach must not
    depend on the rounding family"""
    gemm_form = {(name, args) for name, args, _ in table if name in GEMM_FORM}
    exact = tc.selected_instantiations([c for c in all_cases() if c["family"] == "exact"])
    assert not gemm_form - exact, sorted(gemm_form - exact)
    assert len(gemm_form) == 24 + 16


def test_two_workgroups_fit_a_compute_unit(table):
    two_per_cu = kernels_with_two_waves_per_eu()
    assert two_per_cu == {"conv3x3_kernel"}
    for name, args, f in table:
        assert f["vgpr"] <= 256, (name, args)
        if name in two_per_cu:
            assert f["lds"] <= LDS_PER_CU // 2, (name, args, f["lds"])


def render(table):
    reach = {}
    for c in all_cases():
        for k in c["kernels"]:
            r = reach.setdefault(k, {"round": 0, "exact": 0, "regime": 0})
            r[c["family"]] += 1
    lines = ["# Template instantiations of csrc/conv_nhwc.hip", "",
             "Compiled for gfx950 with the Makefile's flags (`-O3 -ffp-contract=off`); produced by",
             "`python tests/test_image_pyramid_instantiations_cpu.py`.  The case columns count the C-ABI cases of",
             "`tests/image_pyramid_cases.py` and `tests/image_pyramid_train_cases.py` that launch the kernel by the restated dispatch",
             "rules: the rounding family (a derived bound), the exact family (bit for bit) and the launch-regime cases (exact inputs at",
             "production grid sizes).  The NT = 8 forms of `conv3x3_kernel` spill; nothing else does.", "",
             "| kernel | template arguments | LDS bytes | VGPRs | spilled VGPRs | spilled SGPRs | scratch bytes | rounding | exact | regime |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for name, args, f in table:
        r = reach.get((name, args), {"round": 0, "exact": 0, "regime": 0})
        lines.append("| `%s` | %s | %d | %d | %d | %d | %d | %d | %d | %d |" % (
            name, ", ".join(str(a).lower() for a in args) or "-", f["lds"], f["vgpr"], f["spill"], f["sgpr_spill"], f["scratch"], r["round"],
            r["exact"], r["regime"]))
    lines += ["", "%d kernels, %d cases." % (len(table), len(all_cases()))]
    return "\n".join(lines)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(render(kernel_table(compile_to_assembly(d, SOURCE))))
