"""Coverage guard of the glue parity suite, on any machine with hipcc: csrc/glue.hip is compiled to assembly with the Makefile's flags, and
the instantiations of the codec, projection and concat kernels in the code object must equal the set that the cases of
tests/glue_cases.py reach by the restated launch rule.  A new VEC width cannot land without a case, and a case table that stops reaching
one fails here without a GPU.  The other kernels of the file are only listed: the loss kernels belong to tests/loss_cases.py, the
ordered-scatter kernels to tests/ordered_grad_cases.py.  Only symbol names are read from the assembly."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_cases as gc  # noqa: E402
from kernel_asm import compile_to_assembly  # noqa: E402

LOSS_KERNELS = {"rpn_loss_kernel", "rpn_loss_finalize_kernel", "rcnn_loss_kernel", "rcnn_loss_finalize_kernel"}


def kernel_symbols(text):
    """the names of the kernels in the metadata of the assembly"""
    return sorted(set(re.findall(r"^\s*\.name:\s+(_Z\w+)\s*$", text, re.M)) & set(re.findall(r"^\s*\.amdhsa_kernel\s+(\w+)", text, re.M)))


def parse(symbol):
    """_ZN2hf<len><name>[ILi<n>E]E... -> (name, template arguments) for a kernel of namespace hf with at most one integer argument;
    None for any other symbol"""
    m = re.match(r"_ZN2hfL?(\d+)", symbol)           # L: a kernel with internal linkage
    if not m:
        return None
    name = symbol[m.end():m.end() + int(m.group(1))]
    rest = symbol[m.end() + int(m.group(1)):]
    t = re.match(r"ILi(\d+)EE", rest)
    if t:
        return name, (int(t.group(1)),)
    return (name, ()) if rest.startswith("E") else (name, None)


@pytest.fixture(scope="module")
def symbols(tmp_path_factory):
    return kernel_symbols(compile_to_assembly(tmp_path_factory.mktemp("glue_asm"), "glue.hip"))


def test_parse():
    assert parse("_ZN2hf21project_gather_kernelILi4EEEviiiixPKfS2_S2_PfPi") == ("project_gather_kernel", (4,))
    assert parse("_ZN2hf21bin_box_encode_kernelExiiPKfS1_S1_S1_S1_S1_S1_ffffPiPfS2_S3_S2_S3_S3_S3_") == ("bin_box_encode_kernel", ())
    assert parse("_ZN2hf15rpn_loss_kernelILb1EEEvNS_8LossArgsEPfPKfS4_S2_S2_")[0] == "rpn_loss_kernel"


def test_the_compiled_instantiations_are_those_the_case_table_reaches(symbols):
    parsed = [parse(s) for s in symbols]
    assert all(parsed), [s for s, p in zip(symbols, parsed) if not p]
    compiled = {p for p in parsed if p[0] in gc.KERNELS}
    reached = gc.reached_instantiations()
    assert not compiled - reached, "compiled but reached by no case of glue_cases.py: %s" % sorted(compiled - reached)
    assert not reached - compiled, "the launch rule restated in glue_cases.py names kernels that do not exist: %s" % sorted(reached - compiled)
    assert {name for name, _ in compiled} == set(gc.KERNELS) and len(compiled) == 10
    others = {p[0] for p in parsed} - set(gc.KERNELS)
    print("kernels of glue.hip that belong to other suites: %s" % sorted(others))
    assert LOSS_KERNELS <= others, "the loss kernels (tests/loss_cases.py) are expected in the same code object"
