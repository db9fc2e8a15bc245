"""K split of the wide single-precision products (chase_hip_gemm_sd / _cz and their bf16x3 twins) under gemm_min_rounds, the part
that needs no GPU: the host-only plan query (chase_hip_gemm_sp_plan, chase_hip_gemm_sp_workspace_bytes) follows the rule the header
states, and the kernels, cross-compiled to gfx950 assembly: the reduction kernel uses no scratch and spills nothing, the wide
product kernels take their piece from the second grid dimension and the narrow ones do not.

The rule (sp_frame::split_plan): slots = 2 num_cu.  No split with min_rounds <= 0, and none for a launch of a whole round and
more (tiles >= slots; in particular none with tiles >= min_rounds slots).  A smaller launch counts its work in 128 x 64 tiles (a
128-column tile holds its workgroup slot twice as long - the count of sp_frame::tile_cols): sk = ceil(min_rounds slots / that
count), at most 8, at most k // min_piece_k (64 K steps of the kernel: 1024 k, complex fp32 512), at most what the workspace cap
holds; kchunk = ceil(k / sk) rounded up to 16."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KINDS = [(split, cplx, op) for split in (False, True) for cplx in (False, True) for op in ("N", "C")]
KIND_IDS = [("bf16x3" if s else "fp32") + ("-z" if c else "-d") + o for (s, c, o) in KINDS]
NUM_CU = 256


def plan(split, cplx, op, m, n, k, min_rounds, num_cu=NUM_CU):
    from chase_amd import capi
    return capi.gemm_sp_plan(cplx, op, m, n, k, split=split, num_cu=num_cu, min_rounds=min_rounds)


def test_library_header_and_binding_have_the_entry_points():
    names = ("chase_hip_gemm_sp_plan", "chase_hip_gemm_sp_workspace_bytes", "chase_hip_ctx_gemm_sp_counters")
    lib = ctypes.CDLL(os.path.join(ROOT, "chase_amd", "lib", "libchase_hip.so"))
    assert not [n for n in names if not hasattr(lib, n)]
    hdr = open(os.path.join(ROOT, "include", "chase_hip.h")).read()
    assert all(re.search(r"\b%s\s*\(" % n, hdr) for n in names)
    fields = re.search(r"typedef struct chase_hip_gemm_sp_launch \{(.*?)\}", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", fields) == ["bn", "gm", "gn", "sk", "kchunk", "min_piece_k", "slab_bytes"]
    from chase_amd import capi
    assert [f for f, _ in capi.GemmSpLaunch._fields_] == ["bn", "gm", "gn", "sk", "kchunk", "min_piece_k", "slab_bytes"]
    assert all(getattr(capi.lib, n).argtypes for n in names)
    assert callable(capi.Context.gemm_sp_counters) and callable(capi.Context.set_gemm_min_rounds)


@pytest.mark.parametrize("split,cplx,op", KINDS, ids=KIND_IDS)
def test_no_split_when_off_or_filled(split, cplx, op):
    mp = plan(split, cplx, op, 130, 70, 1, 0)["min_piece_k"]
    assert mp == (512 if cplx and not split else 1024)             # 64 K steps of 8 (complex fp32) or 16 k
    # min_rounds = 0: whole K whatever the shape - ragged, the losing 2 x 2 panel, the panels of a 4 x 2 rank of config 4
    # (N = 65536: 16384 x 32768 and 32768 x 16384 local blocks, 256 columns), full width
    shapes = [(130, 70, 8 * mp + 37), (4096, 128, 4096), (16384, 256, 32768), (32768, 256, 16384), (16384, 2560, 32768),
              (1, 1, 1 << 20), (128, 64, 16 * mp)]
    for (m, n, k) in shapes:
        p = plan(split, cplx, op, m, n, k, 0)
        assert p["sk"] == 1 and p["slab_bytes"] == 0, (m, n, k, p)
        assert p["gm"] == -(-m // 128) and p["gn"] == -(-n // p["bn"]) and p["bn"] in (64, 128)
    # min_rounds > 0 and the launch has min_rounds tiles per workgroup slot already: whole K
    for (m, n, k, r, cu) in [(16384, 2048, 8 * mp, 4, 256), (16384, 1024, 8 * mp, 2, 256), (1024, 1024, 8 * mp, 4, 8),
                             (65536, 2560, 65536, 4, 256), (8192, 128, 8 * mp, 1, 32)]:
        p = plan(split, cplx, op, m, n, k, r, cu)
        assert p["gm"] * p["gn"] >= r * 2 * cu, (m, n, r, cu, p)   # (the case is what it claims to be)
        assert p["sk"] == 1 and p["slab_bytes"] == 0, (m, n, k, r, cu, p)
    # a whole round of workgroups is not cut either (measured: it loses to the slab traffic), one tile fewer is
    p = plan(split, cplx, op, 128 * 64, 64, 8 * mp, 4, 32)
    assert p["bn"] == 64 and p["gm"] * p["gn"] == 64 and p["sk"] == 1
    p = plan(split, cplx, op, 128 * 63, 64, 8 * mp, 1, 32)
    assert p["bn"] == 64 and p["gm"] * p["gn"] == 63 and p["sk"] == 2
    p = plan(split, cplx, op, 128 * 63, 64, 8 * mp, 4, 32)
    assert p["gm"] * p["gn"] == 63 and p["sk"] == 5                # ceil(4 * 64 / 63)


@pytest.mark.parametrize("split,cplx,op", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("min_rounds", [4, 16])
def test_split_arithmetic_of_a_ragged_product(split, cplx, op, min_rounds):
    m, n = 130, 70
    mp = plan(split, cplx, op, m, n, 1, min_rounds)["min_piece_k"]
    for s in (1, 2, 3, 8, 9):
        for r in (0, 37):
            k = mp * s + r
            p = plan(split, cplx, op, m, n, k, min_rounds)
            sk, kc = p["sk"], p["kchunk"]
            assert sk == (1 if s == 1 else min(8, s)), (s, r, p)
            assert p["bn"] == 64 and p["gm"] == 2 and p["gn"] == 2
            if sk == 1:
                assert p["slab_bytes"] == 0
                continue
            assert kc % 16 == 0
            assert (sk - 1) * kc < k <= sk * kc, (s, r, p)             # pieces cover [0, k) exactly, none is empty
            assert p["slab_bytes"] == sk * p["gm"] * 128 * p["gn"] * p["bn"] * 8 * (2 if cplx else 1)
    # one k below two minimum pieces: whole K
    assert plan(split, cplx, op, m, n, 2 * mp - 1, min_rounds)["sk"] == 1


@pytest.mark.parametrize("op", ["N", "C"])
def test_panels_of_the_design_document(op):
    """the grid filter's default product (fp32 MFMA), complex, 256 CUs, min_rounds = 4: the 2 x 2 panel that lost against fp64
    (4096 x 4096 local block, 128 columns: 64 tiles of 128 x 64) is cut 8 ways, the panel of a 4 x 2 rank of N = 65536
    (256 tiles of 128 x 128 = 512 of 128 x 64) 4 ways.  The bf16x3 product of the first panel has half as many 16-k steps:
    4096 / 1024 = 4 pieces; that of the second one is 512 tiles of 128 x 64, a whole round of workgroups: not cut."""
    p = plan(False, True, op, 4096, 128, 4096, 4)
    assert (p["bn"], p["gm"] * p["gn"], p["sk"], p["kchunk"]) == (64, 64, 8, 512)
    p = plan(False, True, op, 16384, 256, 32768, 4)
    assert (p["bn"], p["gm"] * p["gn"], p["sk"], p["kchunk"]) == (128, 256, 4, 8192)
    assert p["slab_bytes"] == 4 * 16384 * 256 * 16
    p = plan(True, True, op, 4096, 128, 4096, 4)
    assert (p["bn"], p["sk"], p["kchunk"]) == (64, 4, 1024)
    p = plan(True, True, op, 16384, 256, 32768, 4)
    assert (p["bn"], p["gm"] * p["gn"], p["sk"]) == (64, 512, 1)


@pytest.mark.parametrize("split,cplx,op", KINDS, ids=KIND_IDS)
def test_workspace_covers_the_plan_and_the_query_is_pure(split, cplx, op):
    from chase_amd import capi
    cap = 640 << 20
    for (m, n, k, r, cu) in [(130, 70, 8229, 4, 256), (4096, 128, 4096, 4, 256), (16384, 256, 32768, 4, 256), (16384, 256, 16384, 16, 256),
                             (65536, 256, 65536, 16, 256), (257, 129, 3000, 4, 304), (4096, 128, 4096, 0, 256), (0, 5, 4096, 4, 256)]:
        a = plan(split, cplx, op, m, n, k, r, cu)
        ws = capi.gemm_sp_workspace_bytes(cplx, op, m, n, k, split=split, num_cu=cu, min_rounds=r)
        assert ws >= a["slab_bytes"] and ws <= cap, (m, n, k, r, cu, a, ws)
        assert (a["slab_bytes"] == 0) == (a["sk"] == 1)
        for _ in range(3):                                          # no state: the same answer every time, whatever was asked between
            plan(not split, not cplx, "N", 4096, 128, 4096, 4)
            assert plan(split, cplx, op, m, n, k, r, cu) == a
            assert capi.gemm_sp_workspace_bytes(cplx, op, m, n, k, split=split, num_cu=cu, min_rounds=r) == ws
    # the workspace cap limits the pieces of a large panel: 511 complex tiles of 128 x 128 are 128 MB a piece, 8 do not fit
    big = plan(False, True, op, 65408, 128, 65536, 16)
    assert (big["bn"], big["gm"] * big["gn"], big["sk"]) == (128, 511, 5) and big["slab_bytes"] == 5 * 65408 * 128 * 16 <= cap
    out = capi.GemmSpLaunch()
    assert capi.lib.chase_hip_gemm_sp_plan(0, int(cplx), b"X", 8, 8, 8, 256, 0, ctypes.byref(out)) == -1001      # CHASE_HIP_EINVAL
    assert capi.lib.chase_hip_gemm_sp_plan(0, int(cplx), op.encode(), 8, 8, -1, 256, 0, ctypes.byref(out)) == -1001


def _compile(tmp_path, name):
    src = os.path.join(ROOT, "chase_amd", "csrc", name)
    out = tmp_path / (name + ".s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "chase_amd", "csrc"), "-S", "--cuda-device-only", "-o",
                        str(out), src], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    asm = out.read_text()
    desc = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", asm, re.S)}
    return asm, desc


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_reduction_kernel_uses_no_scratch_and_spills_nothing(tmp_path):
    asm, desc = _compile(tmp_path, "vec_kernels.hip")
    red = {k: d for k, d in desc.items() if "sp_slab_reduce_kernel" in k}
    assert len(red) == 2, sorted(desc)                             # real and complex
    for name, d in red.items():
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", d).group(1)) == 0, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", d).group(1)) == 0, name
        # its record in the code-object metadata: no private segment, no spilled register
        # (the keys of a record are sorted: those after .name up to the record's last, .wavefront_size)
        rec = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size:" % re.escape(name), asm[asm.index("amdhsa.kernels"):], re.S).group(1)
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", rec).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s*(\d+)", rec).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", rec).group(1)) == 0, name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
@pytest.mark.parametrize("name", ["gemm_mfma_f32.hip", "gemm_mfma_bf16x3.hip"])
def test_wide_kernels_take_their_piece_from_the_second_grid_dimension(tmp_path, name):
    """a K piece is workgroup (tile, piece) of an ordinary launch: the wide kernels (last template argument) read the workgroup
    id along y, the narrow ones - never cut - do not; no kernel beside the product kernels lives in these files"""
    asm, desc = _compile(tmp_path, name)
    assert desc and all(re.search(r"gemm_(f32|bf16x3)_kernel", k) for k in desc), sorted(desc)
    wide = 0
    for k, d in desc.items():
        args = re.search(r"kernelIL(b[01])EL(i\d)EL(i\d)EL(b[01])EL(b[01])EE", k)
        assert args, k
        is_wide = args.group(5) == "b1"
        wide += is_wide
        assert int(re.search(r"\.amdhsa_system_sgpr_workgroup_id_y (\d)", d).group(1)) == int(is_wide), k
    assert 0 < wide < len(desc)
