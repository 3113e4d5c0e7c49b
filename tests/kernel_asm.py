"""Reading the kernels of a csrc/*.hip file from its gfx950 assembly, on any machine with hipcc: the file is compiled with the Makefile's
flags and the .amdgpu_metadata of the result gives every kernel's template arguments and resources.  A plain module, shared by the
tests/test_*_instantiations_cpu.py coverage guards and the resource checks of the bf16 files."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heterofusionrcnn_amd", "csrc")
LDS_PER_CU = 160 * 1024


def compile_to_assembly(directory, source="gemm.hip"):
    asm = os.path.join(str(directory), os.path.splitext(source)[0] + ".s")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17",
                    "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-S", os.path.join(CSRC, source), "-o", asm],
                   check=True, capture_output=True)
    with open(asm) as f:
        return f.read()


def demangle(symbol):
    """_ZN2hf<len><name>[I<L i|b value E>...E]E... -> (name, template arguments); the kernels live in namespace hf and take integer
    and boolean template arguments only"""
    m = re.match(r"_ZN2hf(\d+)", symbol)
    assert m, symbol
    start = m.end()
    name = symbol[start:start + int(m.group(1))]
    rest = symbol[start + int(m.group(1)):]
    args = []
    if rest.startswith("I"):
        pos = 1
        while rest[pos] != "E":
            t = re.match(r"L([ib])(n?\d+)E", rest[pos:])
            assert t, symbol
            args.append(bool(int(t.group(2))) if t.group(1) == "b" else int(t.group(2).replace("n", "-")))
            pos += t.end()
    return name, tuple(args)


def kernel_table(text):
    """[(kernel, template arguments, metadata fields)] from the .amdgpu_metadata of the assembly"""
    rows = []
    for blk in re.split(r"\n\s*- \.agpr_count", text)[1:]:
        symbol = re.search(r"\.name:\s+(\S+)", blk).group(1)
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
        name, args = demangle(symbol)
        rows.append((name, args, dict(lds=field("group_segment_fixed_size"), vgpr=field("vgpr_count"), spill=field("vgpr_spill_count"),
                                      sgpr_spill=field("sgpr_spill_count"), scratch=field("private_segment_fixed_size"))))
    return sorted(rows, key=lambda r: (r[0], r[1]))
