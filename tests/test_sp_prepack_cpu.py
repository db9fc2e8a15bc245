"""bf16x3 product on a packed H (sp_prepack = 1), the part that needs no GPU: the library exports the five entry points and the
binding declares them; the solver header documents the key; the numpy restatement of the packed layout (tests/bf16x3_pack_ref.py)
is a bijection that gives the split back; and chase_amd/csrc/gemm_mfma_bf16x3p.hip, cross-compiled to gfx950 assembly, keeps the
32x32x16 bf16 MFMA in every product kernel, uses no scratch and fits the registers and the LDS its launch bounds promise (asserts
on kernel descriptors and metadata; the only instruction looked for is the MFMA)."""
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
import bf16x3_pack_ref as PR  # noqa: E402
import bf16x3_ref as R  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW_SYMBOLS = ("chase_hip_bf16x3_pack_bytes", "chase_hip_bf16x3_pack", "chase_hip_bf16x3_pack_diag", "chase_hip_gemm_s_bf16x3p",
               "chase_hip_gemm_c_bf16x3p")


def test_library_exports_the_packed_product_entry_points():
    lib = ctypes.CDLL(os.path.join(ROOT, "chase_amd", "lib", "libchase_hip.so"))
    missing = [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert not missing, missing
    hdr = open(os.path.join(ROOT, "include", "chase_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in NEW_SYMBOLS)


def test_binding_declares_the_packed_product_entry_points():
    from chase_amd import capi
    c = ctypes
    want = {
        "chase_hip_bf16x3_pack_bytes": [c.c_int, c.c_int, c.c_int, c.POINTER(c.c_size_t)],
        "chase_hip_bf16x3_pack": [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_long, c.c_void_p],
        "chase_hip_bf16x3_pack_diag": [c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_long, c.c_void_p],
        "chase_hip_gemm_s_bf16x3p": [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_float, c.c_void_p, c.c_void_p, c.c_long, c.c_float,
                                     c.c_void_p, c.c_long],
        "chase_hip_gemm_c_bf16x3p": [c.c_void_p, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_float), c.c_void_p, c.c_void_p, c.c_long,
                                     c.POINTER(c.c_float), c.c_void_p, c.c_long],
    }
    for n, args in want.items():
        fn = getattr(capi.lib, n)
        assert fn.restype is c.c_int and list(fn.argtypes) == args, n
    for f in ("bf16x3_pack_bytes", "bf16x3_pack", "bf16x3_pack_diag", "gemm32p"):
        assert inspect.isfunction(getattr(capi.Context, f)), f
    # the size query needs no device
    b = c.c_size_t(7)
    for cplx, m, k, bytes_ in ((0, 1, 1, 3 * 4096), (1, 1, 1, 6 * 4096), (0, 129, 17, 2 * 2 * 3 * 4096), (1, 300, 300, 3 * 19 * 6 * 4096),
                               (0, 0, 5, 0), (1, 5, 0, 0)):
        assert capi.lib.chase_hip_bf16x3_pack_bytes(cplx, m, k, c.byref(b)) == 0
        assert b.value == bytes_ == PR.pack_bytes(m, k, bool(cplx)), (cplx, m, k, b.value)


def test_solver_header_and_source_know_the_key():
    hdr = open(os.path.join(ROOT, "include", "chase_hip_solver.h")).read()
    for word in ("sp_prepack", "CHASE_HIP_SP_PREPACK", "hemm_sp_packed_calls", "sp_pack_full", "sp_pack_diag"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "chase_amd", "host", "solver_capi.cpp")).read()
    assert "solver_set: sp_prepack" in src


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("m,k", [(1, 1), (128, 16), (129, 17), (5, 11), (300, 300), (257, 1000)])
def test_pack_ref_is_a_bijection_and_gives_the_split_back(m, k, cplx):
    rng = np.random.default_rng(1000 * m + k + cplx)
    A = rng.standard_normal((m, k)).astype(np.float32)
    if cplx:
        A = (A + 1j * rng.standard_normal((m, k))).astype(np.complex64)
    P, T = PR.dims(m, k)
    idx = PR._index(m, k, cplx)
    assert idx.shape == (PR.planes(cplx), 128 * P, 16 * T)
    assert np.array_equal(np.sort(idx.ravel()), np.arange(PR.pack_bytes(m, k, cplx) // 2))        # onto the padded buffer, one to one
    buf = PR.pack(A)
    assert buf.dtype == np.uint8 and buf.size == PR.pack_bytes(m, k, cplx)
    parts, padding = PR.unpack(buf, m, k, cplx)
    assert not np.any(padding)
    want = PR.part_planes(A)
    assert parts.tobytes() == want.tobytes()
    comps = (A.real, A.imag) if cplx else (A,)
    for c, x in enumerate(comps):
        s = (parts[3 * c].astype(np.float64) + parts[3 * c + 1].astype(np.float64)) + parts[3 * c + 2].astype(np.float64)
        assert np.array_equal(s, x.astype(np.float64))                      # the three parts are the number
        assert tuple(p.tobytes() for p in parts[3 * c:3 * c + 3]) == tuple(p.tobytes() for p in R.split3(np.ascontiguousarray(x)))
    # a piece is 8 consecutive k of one row: element (0, 0) of part 1 leads piece 0, (0, 8) piece 1, (4, 0) piece 9 (swizzled)
    assert idx[0, 0, 0] == 0 and idx[0, 0, 8] == 8 and idx[0, 4, 0] == 8 * 9 and idx[0, 4, 8] == 8 * 8 and idx[0, 12, 0] == 8 * 24
    assert idx[1, 0, 0] == 8 * 256 and (T == 1 or idx[0, 0, 16] == 8 * 256 * PR.planes(cplx))       # next plane, next K step


def test_pack_of_nothing_is_empty():
    assert PR.pack(np.zeros((0, 5), np.float32)).size == 0 and PR.pack(np.zeros((5, 0), np.complex64)).size == 0


def in_a_loop(lines, k):
    """the basic block of line k belongs to a loop: the compiler annotates every block of a loop on the block's label line"""
    for i in range(k, -1, -1):
        if re.match(r"(\.LBB\w+:|; %bb\.\d+:)", lines[i]):
            return "Loop" in lines[i]
    return False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_packed_product_kernels_keep_the_bf16_mfma_in_the_loop_and_fit_their_resources(tmp_path):
    src = os.path.join(ROOT, "chase_amd", "csrc", "gemm_mfma_bf16x3p.hip")
    out = tmp_path / "gemm_bf16x3p.s"
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "chase_amd", "csrc"), "-S", "--cuda-device-only", "-o",
                        str(out), src], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    asm = out.read_text()
    desc = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)}
    product = {k: d for k, d in desc.items() if "gemm_bf16x3p_kernel" in k}
    pack = {k: d for k, d in desc.items() if "bf16x3_pack_kernel" in k}
    diag = {k: d for k, d in desc.items() if "bf16x3_pack_diag_kernel" in k}
    # product: real 2 tile widths x 2 tags, complex one tile width x 2 tags; pack: real / complex x fp32 / fp64; diag: real / complex
    assert len(product) == 6 and len(pack) == 4 and len(diag) == 2 and len(desc) == 12, sorted(desc)
    src_text = open(src).read()
    body = src_text[src_text.index("void gemm_bf16x3p_kernel") - 200:]
    bounds = re.search(r"__launch_bounds__\((\d+),\s*(\d+)\)\s*void gemm_bf16x3p_kernel", body)
    threads, blocks_per_cu = int(bounds.group(1)), int(bounds.group(2))
    assert (threads, blocks_per_cu) == (256, 2)                            # the promise of gemm_mfma_bf16x3.hip
    budget = int(512 / (threads // 64 * blocks_per_cu / 4.0))              # unified VGPR file: 512 registers per lane and SIMD
    for name, d in desc.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d).group(1)) == 0, name      # no scratch
        vg = int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", d).group(1))
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", d).group(1))
        if name not in product:
            assert vg <= 128 and lds == 0, (name, vg, lds)                 # streaming kernels: 256 threads, no LDS
            continue
        assert vg <= budget, (name, vg, budget)
        assert 0 < lds and lds * blocks_per_cu <= 160 * 1024, (name, lds)
        m = re.search(r"^%s:[^\n]*\n" % re.escape(name), asm, re.M)
        lines = asm[m.end():asm.index(".Lfunc_end", m.end())].split("\n")
        mfma = [k for k, l in enumerate(lines) if re.match(r"\s*v_mfma_", l)]
        assert mfma, name
        assert all(re.match(r"\s*v_mfma_f32_32x32x16_bf16\b", lines[k]) for k in mfma), name        # no other matrix instruction
        assert any(in_a_loop(lines, k) for k in mfma), name
    # the LDS of a product kernel is that of the kernel it restates: (3 or 6 planes) x (128 + BN rows) x 32 bytes x 2 buffers
    assert sorted(int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", d).group(1)) for d in product.values()) == \
        sorted([2 * 3 * 32 * 192] * 2 + [2 * 3 * 32 * 256] * 2 + [2 * 6 * 32 * 192] * 2)
    # the code-object metadata agrees: no private segment, nothing spilled
    meta = asm[asm.index("amdhsa.kernels"):]
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", meta)
    assert len(sizes) == len(desc) and all(int(x) == 0 for x in sizes), sizes
    assert all(int(x) == 0 for x in re.findall(r"\.vgpr_spill_count:\s*(\d+)", meta))
    assert all(int(x) == 0 for x in re.findall(r"\.sgpr_spill_count:\s*(\d+)", meta))
