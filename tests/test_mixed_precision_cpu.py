"""Mixed-precision filter, the part that needs no GPU: the library exports the new entry points, and the fp32 MFMA GEMM
(chase_amd/csrc/gemm_mfma_f32.hip), cross-compiled to gfx950 assembly, keeps its matrix-core instructions in the K loop, fits the
registers its launch bounds promise and uses no scratch.  Asserts on kernel descriptors and metadata; the only instruction looked
for is the MFMA."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("chase_hip_gemm_s", "chase_hip_gemm_c", "chase_hip_convert_d2s", "chase_hip_convert_s2d", "chase_hip_diag_d2s")


def test_library_exports_the_single_precision_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "chase_amd", "lib", "libchase_hip.so"))
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "chase_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in NEW_SYMBOLS)


def test_binding_declares_the_new_entry_points():
    from chase_amd import capi
    for n in NEW_SYMBOLS:
        assert getattr(capi.lib, n).argtypes, n
    assert callable(capi.Context.gemm32) and callable(capi.Context.convert_d2s) and callable(capi.Context.diag_d2s)


def in_a_loop(lines, k):
    """the basic block of line k belongs to a loop: the compiler annotates every block of a loop on the block's label line"""
    for i in range(k, -1, -1):
        if re.match(r"(\.LBB\w+:|; %bb\.\d+:)", lines[i]):
            return "Loop" in lines[i]
    return False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_f32_gemm_kernels_keep_mfma_in_the_loop_and_fit_their_registers(tmp_path):
    src = os.path.join(ROOT, "chase_amd", "csrc", "gemm_mfma_f32.hip")
    out = tmp_path / "gemm32.s"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "chase_amd", "csrc"), "-S", "--cuda-device-only", "-o",
                        str(out), src], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    asm = out.read_text()
    # every kernel the file defines, from the descriptors
    desc = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)}
    assert len(desc) >= 8 and all("gemm_f32_kernel" in k for k in desc), sorted(desc)     # real / complex x tile width x tag
    src_text = open(src).read()
    bounds = re.search(r"__launch_bounds__\((\d+),\s*(\d+)\)", src_text)
    threads, blocks_per_cu = int(bounds.group(1)), int(bounds.group(2))
    waves_per_simd = threads // 64 * blocks_per_cu / 4.0
    budget = int(512 / waves_per_simd)                     # unified VGPR file: 512 registers per lane and SIMD
    for name, d in desc.items():
        vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", d).group(1))
        assert vg <= budget, (name, vg, budget)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d).group(1)) == 0, name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", d).group(1))
        assert lds * blocks_per_cu <= 160 * 1024, (name, lds)
        m = re.search(r"^%s:[^\n]*\n" % re.escape(name), asm, re.M)
        lines = asm[m.end():asm.index(".Lfunc_end", m.end())].split("\n")
        mfma = [k for k, l in enumerate(lines) if "v_mfma_f32_" in l]
        assert mfma, name
        assert any(in_a_loop(lines, k) for k in mfma), name
    # the code-object metadata agrees: no private segment, nothing spilled
    meta = asm[asm.index("amdhsa.kernels"):]
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", meta)
    assert len(sizes) == len(desc) and all(int(x) == 0 for x in sizes), sizes
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", meta))
