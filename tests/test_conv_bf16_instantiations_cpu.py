"""Coverage guard of the bf16 convolution's parity suite, on any machine with hipcc: csrc/conv_nhwc_bf16.hip is compiled to assembly
with the Makefile's flags, and the set of kernels in the code object must equal the set of template instantiations that the C-ABI
cases of tests/conv_bf16_cases.py select by the restated dispatch rule.  Only kernel names and the resource fields of the metadata
are read.  Run as a script, the module prints the resource table committed as profiles/conv_nhwc_bf16_instantiations.md."""
import os
import re
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bf16_cases as cb  # noqa: E402
from kernel_asm import CSRC, LDS_PER_CU, compile_to_assembly, kernel_table  # noqa: E402


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return kernel_table(compile_to_assembly(tmp_path_factory.mktemp("conv_nhwc_bf16_asm"), cb.SOURCE))


def test_every_compiled_instantiation_is_selected_by_a_case_and_nothing_else(table):
    compiled = {(name, args) for name, args, _ in table}
    selected = cb.selected_instantiations()
    assert not compiled - selected, "compiled but reached by no case: %s" % sorted(compiled - selected)
    assert not selected - compiled, "the restated dispatch rule names kernels that do not exist: %s" % sorted(selected - compiled)
    assert len(table) == len(compiled) == 16       # four column tiles x {vector, scalar staging} x {plain, up}


def test_exact_family_alone_reaches_every_instantiation(table):
    """every kernel of the file is GEMM-form; the bit-for-bit family is the one that sees a dropped product, a stale prefetch or a
    wrong tap of a parity class at any summation order"""
    compiled = {(name, args) for name, args, _ in table}
    exact = cb.selected_instantiations([c for c in cb.abi_cases() if c["family"] == "exact"])
    assert not compiled - exact, sorted(compiled - exact)


def test_resources(table):
    """256 VGPRs, no spill, no scratch; amdgpu_waves_per_eu(2) claims two workgroups per CU wherever a workgroup is four waves: half
    the CU's LDS each"""
    with open(os.path.join(CSRC, cb.SOURCE)) as f:
        assert set(re.findall(r"amdgpu_waves_per_eu\(2\)\)\)\s*void\s+(\w+)\s*\(", f.read())) == {"conv3x3_bf16_kernel"}
    for name, args, f in table:
        assert f["vgpr"] <= 256 and f["spill"] == 0 and f["sgpr_spill"] == 0 and f["scratch"] == 0, (name, args, f)
        assert f["lds"] <= LDS_PER_CU // 2 == 80 * 1024, (name, args, f["lds"])


def render(table):
    reach = {}
    for c in cb.abi_cases():
        for k in c["kernels"]:
            reach.setdefault(k, {"round": 0, "exact": 0, "regime": 0})[c["family"]] += 1
    lines = ["# Template instantiations of csrc/conv_nhwc_bf16.hip", "",
             "Compiled for gfx950 with the Makefile's flags (`-O3 -ffp-contract=off`); produced by",
             "`python tests/test_conv_bf16_instantiations_cpu.py`.  Template arguments: NT, WN (the column tile is 16 NT WN), vector staging,",
             "up-convolution.  The case columns count the C-ABI cases of `tests/conv_bf16_cases.py` that launch the kernel by the restated",
             "dispatch rule: the rounding family (a derived bound), the exact family (bit for bit) and the launch-regime cases.  Nothing spills.", "",
             "| kernel | template arguments | LDS bytes | VGPRs | spilled VGPRs | spilled SGPRs | scratch bytes | rounding | exact | regime |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for name, args, f in table:
        r = reach.get((name, args), {"round": 0, "exact": 0, "regime": 0})
        lines.append("| `%s` | %s | %d | %d | %d | %d | %d | %d | %d | %d |" % (
            name, ", ".join(str(a).lower() for a in args), f["lds"], f["vgpr"], f["spill"], f["sgpr_spill"], f["scratch"], r["round"],
            r["exact"], r["regime"]))
    lines += ["", "%d kernels, %d cases." % (len(table), len(cb.abi_cases()))]
    return "\n".join(lines)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(render(kernel_table(compile_to_assembly(d, cb.SOURCE))))
