"""bf16x3 split product of the mixed-precision filter, the part that needs no GPU: the library exports the four entry points and
the binding declares them; chase_amd/csrc/gemm_mfma_bf16x3.hip, cross-compiled to gfx950 assembly, keeps the 32x32x16 bf16 MFMA
in its K loop, fits the registers and the LDS its launch bounds promise and uses no scratch (asserts on kernel descriptors and
metadata; the only instruction looked for is the MFMA); and the numpy emulation of the split (tests/bf16x3_ref.py) is exact."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bf16x3_ref as R  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("chase_hip_gemm_s_bf16x3", "chase_hip_gemm_c_bf16x3", "chase_hip_gemm_sd_bf16x3", "chase_hip_gemm_cz_bf16x3")


def test_library_exports_the_split_product_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "chase_amd", "lib", "libchase_hip.so"))
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "chase_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in NEW_SYMBOLS)


def test_binding_declares_the_split_product_entry_points():
    from chase_amd import capi
    for n in NEW_SYMBOLS:
        fn = getattr(capi.lib, n)
        assert fn.argtypes and len(fn.argtypes) == 13, n
        assert list(fn.argtypes) == list(getattr(capi.lib, n[:-len("_bf16x3")]).argtypes), n
    assert capi.lib.chase_hip_gemm_sd_bf16x3.argtypes[5] is ctypes.c_double          # fp64 scalars
    assert capi.lib.chase_hip_gemm_s_bf16x3.argtypes[5] is ctypes.c_float
    for f in (capi.Context.gemm32, capi.Context.gemm32w):
        p = inspect.signature(f).parameters
        assert "split" in p and p["split"].default is False


def test_solver_header_and_source_know_the_key():
    hdr = open(os.path.join(ROOT, "include", "chase_hip_solver.h")).read()
    assert "sp_product" in hdr and "CHASE_HIP_SP_PRODUCT" in hdr and "hemm_sp_split_calls" in hdr
    src = open(os.path.join(ROOT, "chase_amd", "host", "solver_capi.cpp")).read()
    assert "solver_set: sp_product" in src


def in_a_loop(lines, k):
    """the basic block of line k belongs to a loop: the compiler annotates every block of a loop on the block's label line"""
    for i in range(k, -1, -1):
        if re.match(r"(\.LBB\w+:|; %bb\.\d+:)", lines[i]):
            return "Loop" in lines[i]
    return False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_bf16x3_gemm_kernels_keep_the_bf16_mfma_in_the_loop_and_fit_their_resources(tmp_path):
    src = os.path.join(ROOT, "chase_amd", "csrc", "gemm_mfma_bf16x3.hip")
    out = tmp_path / "gemm_bf16x3.s"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "chase_amd", "csrc"), "-S", "--cuda-device-only", "-o",
                        str(out), src], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    asm = out.read_text()
    desc = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)}
    # real: 2 tile widths x 2 tags x (narrow N, wide N, wide C); complex: one tile width
    assert len(desc) == 18 and all("gemm_bf16x3_kernel" in k for k in desc), sorted(desc)
    src_text = open(src).read()
    bounds = sorted(set(re.findall(r"__launch_bounds__\((\d+),\s*(\d+)\)", src_text)))
    assert len(bounds) == 1                                # one promise for every kernel (the file comment quotes it too)
    threads, blocks_per_cu = int(bounds[0][0]), int(bounds[0][1])
    waves_per_simd = threads // 64 * blocks_per_cu / 4.0
    budget = int(512 / waves_per_simd)                     # unified VGPR file: 512 registers per lane and SIMD
    for name, d in desc.items():
        vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", d).group(1))
        assert vg <= budget, (name, vg, budget)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d).group(1)) == 0, name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", d).group(1))
        assert 0 < lds and lds * blocks_per_cu <= 160 * 1024, (name, lds)
        m = re.search(r"^%s:[^\n]*\n" % re.escape(name), asm, re.M)
        lines = asm[m.end():asm.index(".Lfunc_end", m.end())].split("\n")
        mfma = [k for k, l in enumerate(lines) if re.match(r"\s*v_mfma_", l)]
        assert mfma, name
        assert all(re.match(r"\s*v_mfma_f32_32x32x16_bf16\b", lines[k]) for k in mfma), name        # no other matrix instruction
        assert any(in_a_loop(lines, k) for k in mfma), name
    # the code-object metadata agrees: no private segment, nothing spilled
    meta = asm[asm.index("amdhsa.kernels"):]
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", meta)
    assert len(sizes) == len(desc) and all(int(x) == 0 for x in sizes), sizes
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", meta))
    assert all(int(x) == 0 for x in re.findall(r"\.sgpr_spill_count:\s*(\d+)", meta))


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -(1.0 + 2.0 ** -8), 0.0, -0.0],
                 np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, -0.0], np.float32)
    assert R.bf16_rne(x).tobytes() == want.tobytes()


def test_three_term_split_is_exact():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(2_000_000) * 10.0 ** rng.uniform(-25, 25, 2_000_000)).astype(np.float32)
    ints = np.concatenate([rng.integers(-2 ** 24 + 1, 2 ** 24, 2_000_000), [2 ** 24 - 1, -2 ** 24 + 1, 2 ** 23 + 1]]).astype(np.float32)
    zeros = np.array([0.0, -0.0], np.float32)
    for v in (x, ints, zeros):
        a1, a2, a3 = R.split3(v)
        for p in (a1, a2, a3):
            assert np.all((p.view(np.uint32) & 0xFFFF) == 0)                   # bf16 numbers
        s = (a1.astype(np.float64) + a2.astype(np.float64)) + a3.astype(np.float64)
        assert np.array_equal(s, v.astype(np.float64))
        nz = v != 0
        assert np.all(np.abs(a2[nz]) <= 2.0 ** -8 * np.abs(v[nz])) and np.all(np.abs(a3[nz]) <= 2.0 ** -16 * np.abs(v[nz]))
    assert R.split3(zeros)[0].tobytes() == zeros.tobytes()                     # the sign of zero survives in the leading part
    # a 24-bit odd integer whose three parts are all non-zero (the exact-term GPU tests are built from such numbers)
    a1, a2, a3 = R.split3(np.float32(11184811.0))
    assert a1 != 0 and a2 != 0 and a3 != 0


def test_dropped_terms_are_below_a_quarter_ulp_per_term():
    rng = np.random.default_rng(4)
    A = rng.standard_normal((64, 515)).astype(np.float32)
    B = rng.standard_normal((515, 48)).astype(np.float32)
    D = R.dropped_terms(A, B)
    absAB = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    print(f"dropped terms / (u/4 |A||B|): max {np.max(np.abs(D) / (R.U / 4 * absAB)):.2e}")
    assert np.all(np.abs(D) <= R.U / 4 * absAB)
    # and the six kept terms make up the rest of the exact product
    (a1, a2, a3), (b1, b2, b3) = [tuple(p.astype(np.float64) for p in R.split3(X)) for X in (A, B)]
    six = a3 @ b1 + a2 @ b2 + a1 @ b3 + a2 @ b1 + a1 @ b2 + a1 @ b1
    exact = A.astype(np.float64) @ B.astype(np.float64)
    assert np.all(np.abs(exact - (six + D)) <= 1e-13 * absAB)
