"""Mixed-precision filter on the grid, the part that needs no GPU: the library exports the new entry points, the header declares
them, the binding has their argument types, and chase_amd/csrc/gemm_mfma_f32.hip instantiates exactly the kernels that are used
(tests/test_mixed_precision_cpu.py checks the resources of every one of them, the new ones included)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("chase_hip_gemm_sd", "chase_hip_gemm_cz", "chase_hip_diag_list_d2s")


def test_library_exports_the_widened_product_and_the_list_diagonal():
    lib = ctypes.CDLL(os.path.join(ROOT, "chase_amd", "lib", "libchase_hip.so"))
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "chase_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in NEW_SYMBOLS)


def test_binding_declares_the_new_entry_points():
    from chase_amd import capi
    for n in NEW_SYMBOLS:
        assert getattr(capi.lib, n).argtypes, n
    assert capi.lib.chase_hip_gemm_sd.argtypes[5] is ctypes.c_double          # fp64 scalars
    assert callable(capi.Context.gemm32w) and callable(capi.Context.diag_list_d2s)


def test_solver_header_and_error_text_name_the_grid():
    hdr = open(os.path.join(ROOT, "include", "chase_hip_solver.h")).read()
    assert "mixed_precision" in hdr and "grid" in hdr[hdr.index("mixed_precision"):hdr.index("mixed_precision") + 400]
    src = open(os.path.join(ROOT, "chase_amd", "host", "solver_capi.cpp")).read()
    assert "solver_set: mixed_precision" in src


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_f32_gemm_file_instantiates_the_kernels_that_are_used(tmp_path):
    src = os.path.join(ROOT, "chase_amd", "csrc", "gemm_mfma_f32.hip")
    out = tmp_path / "gemm32.s"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "chase_amd", "csrc"), "-S", "--cuda-device-only", "-o",
                        str(out), src], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"\.amdhsa_kernel (\S+)", out.read_text())
    # fp32 C, op N: real / complex x tile width x tag = 8;  fp64 C: op N / C x real / complex x tile width x tag = 16
    assert len(names) == 24 and len(set(names)) == 24, sorted(names)
    assert all("gemm_f32_kernel" in k for k in names)
    text = open(src).read()
    assert len(re.findall(r"__launch_bounds__", text)) == 1 and len(re.findall(r"__global__", text)) == 1
