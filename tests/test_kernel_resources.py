"""The MFMA GEMM kernels must fit their registers: no instantiation of gemm_f64_kernel may touch scratch inside a loop.
The ragged three-multiplication instantiations keep a few VGPRs in scratch, but only parked across the K loops: stored before
them, loaded after them, nothing in any loop (an earlier 3M loop did the same with one register, and the form without it was 3 %
slower on all-ragged launches: profiles/r04_ragged_c_compare.txt).  This test pins the placement: every other instantiation has no
scratch at all, and no scratch instruction of any instantiation sits in a basic block that the compiler marks as part of a loop.
Cross-compiles the file to gfx950 assembly - no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# The plane-fed 3M loop (80 KB of LDS, sum fragments next to 192 accumulators): the four RAGGED 3M instantiations park up to five
# registers (stores before the K loops, loads after them); the whole-tile ones - 99 % of the filter's time - have no scratch at all.
PARKED = ("ILb1ELb1ELi0ELb1ELb1ELb0E", "ILb1ELb1ELi1ELb1ELb1ELb0E",     # <cplx, op=C, tag 0 / 1, ragged, 3M, not narrow>
          "ILb1ELb0ELi0ELb1ELb1ELb0E", "ILb1ELb0ELi1ELb1ELb1ELb0E")     # <cplx, op=N, tag 0 / 1, ragged, 3M, not narrow>


def kernel_bodies(asm):
    for m in re.finditer(r"^(_ZN9chase_hip15gemm_f64_kernel\w+):[^\n]*\n", asm, re.M):
        end = asm.index(".Lfunc_end", m.end())
        yield m.group(1), asm[m.end():end].split("\n")


def in_a_loop(lines, k):
    """the basic block of line k belongs to a loop: the compiler annotates every block of a loop ('; =>This Inner Loop Header',
    ';   in Loop: Header=BBx_y Depth=n') on the block's label line"""
    for i in range(k, -1, -1):
        if re.match(r"(\.LBB\w+:|; %bb\.\d+:)", lines[i]):
            return "Loop" in lines[i]
    return False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_no_gemm_instantiation_spills_inside_a_loop(tmp_path):
    src = os.path.join(ROOT, "chase_amd", "csrc", "gemm_mfma_f64.hip")
    out = tmp_path / "gemm.s"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "chase_amd", "csrc"), "-S", "--cuda-device-only", "-o",
                        str(out), src], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    asm = out.read_text()
    seen = 0
    for name, lines in kernel_bodies(asm):
        seen += 1
        scratch = [k for k, l in enumerate(lines) if re.match(r"\s+(scratch_|buffer_(load|store)\w* .*offen)", l)]
        if any(tag in name for tag in PARKED):
            assert 0 < len(scratch) <= 10, (name, len(scratch))             # stores + loads of the parked registers
        else:
            assert not scratch, (name, [lines[k] for k in scratch[:4]])
        for k in scratch:
            assert not in_a_loop(lines, k), (name, lines[k])
        mfma = [k for k, l in enumerate(lines) if "v_mfma_f64_16x16x4" in l]
        assert len(mfma) >= 48, (name, len(mfma))
        assert any(in_a_loop(lines, k) for k in mfma), name                  # (the detector sees the K loop of every kernel)
    assert seen >= 32                                                        # real / complex x op x tag x ragged x 3M x narrow
    # registers and occupancy from the kernel descriptors: at most 256 VGPRs = two waves per SIMD = two workgroups per CU
    for m in re.finditer(r"\.amdhsa_kernel (_ZN9chase_hip15gemm_f64_kernel\w+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2)).group(1))
        assert vg <= 256, (m.group(1), vg)
