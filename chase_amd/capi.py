"""ctypes binding of include/chase_hip.h (the C ABI of libchase_hip.so).

Fails loudly when the HIP extension is missing — there is deliberately no CPU fallback in the product path.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CHASE_HIP_LIB: another build of the same library (kernel-development variants, scripts/dev_build_variant.sh)
LIB_PATH = os.environ.get("CHASE_HIP_LIB") or os.path.join(_HERE, "lib", "libchase_hip.so")


class ChaseHipError(RuntimeError):
    def __init__(self, code, where, text=""):
        super().__init__(f"{where} failed with status {code}: {text}")
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "chase_amd has no CPU fallback.")
    # torch (when present in the process) bundles its own libamdhip64.so.7 / librccl.so.1; importing it first makes
    # the dynamic linker resolve our NEEDED entries to the same runtime instead of loading a second HIP runtime.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing only
        pass
    return C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)


lib = _load()

c_int, c_long, c_size_t, c_double, c_char, c_void_p = C.c_int, C.c_long, C.c_size_t, C.c_double, C.c_char, C.c_void_p
P = C.POINTER


def _sig(name, restype, *argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


_sig("chase_hip_version", C.c_char_p)
_sig("chase_hip_last_error", C.c_char_p)
_sig("chase_hip_ctx_create", c_int, P(c_void_p), c_int, c_void_p)
_sig("chase_hip_ctx_destroy", c_int, c_void_p)
_sig("chase_hip_ctx_sync", c_int, c_void_p)
_sig("chase_hip_ctx_stream", c_void_p, c_void_p)
_sig("chase_hip_ctx_oplog", c_int, c_void_p, c_int)
_sig("chase_hip_ctx_oplog_text", C.c_char_p, c_void_p)
_sig("chase_hip_device_info", c_int, c_void_p, P(c_int), P(c_int), P(c_size_t), C.c_char_p, c_int)
_sig("chase_hip_device_bus_id", c_int, c_void_p, C.c_char_p, c_int)
_sig("chase_hip_device_count", c_int)
_sig("chase_hip_malloc", c_int, c_void_p, P(c_void_p), c_size_t)
_sig("chase_hip_free", c_int, c_void_p, c_void_p)
_sig("chase_hip_memcpy_h2d", c_int, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("chase_hip_memcpy_d2h", c_int, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("chase_hip_memcpy_d2d", c_int, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("chase_hip_memset", c_int, c_void_p, c_void_p, c_int, c_size_t)
_sig("chase_hip_timer_start", c_int, c_void_p)
_sig("chase_hip_timer_stop", c_int, c_void_p, P(C.c_float))
_sig("chase_hip_gemm_d", c_int, c_void_p, c_char, c_int, c_int, c_int, c_double, c_void_p, c_long, c_void_p, c_long,
     c_double, c_void_p, c_long)
_sig("chase_hip_gemm_z", c_int, c_void_p, c_char, c_int, c_int, c_int, P(c_double), c_void_p, c_long, c_void_p,
     c_long, P(c_double), c_void_p, c_long)
_sig("chase_hip_gemm_s", c_int, c_void_p, c_char, c_int, c_int, c_int, C.c_float, c_void_p, c_long, c_void_p, c_long,
     C.c_float, c_void_p, c_long)
_sig("chase_hip_gemm_c", c_int, c_void_p, c_char, c_int, c_int, c_int, P(C.c_float), c_void_p, c_long, c_void_p,
     c_long, P(C.c_float), c_void_p, c_long)
_sig("chase_hip_gemm_sd", c_int, c_void_p, c_char, c_int, c_int, c_int, c_double, c_void_p, c_long, c_void_p, c_long,
     c_double, c_void_p, c_long)
_sig("chase_hip_gemm_cz", c_int, c_void_p, c_char, c_int, c_int, c_int, P(c_double), c_void_p, c_long, c_void_p,
     c_long, P(c_double), c_void_p, c_long)
for _n in ("s", "c", "sd", "cz"):          # the split-operand (bf16x3) forms have the signatures of the fp32 MFMA ones
    _sig("chase_hip_gemm_%s_bf16x3" % _n, c_int, *getattr(lib, "chase_hip_gemm_" + _n).argtypes)
_sig("chase_hip_bf16x3_pack_bytes", c_int, c_int, c_int, c_int, P(c_size_t))
_sig("chase_hip_bf16x3_pack", c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_long, c_void_p)
_sig("chase_hip_bf16x3_pack_diag", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p)
_sig("chase_hip_gemm_s_bf16x3p", c_int, c_void_p, c_int, c_int, c_int, C.c_float, c_void_p, c_void_p, c_long, C.c_float, c_void_p,
     c_long)
_sig("chase_hip_gemm_c_bf16x3p", c_int, c_void_p, c_int, c_int, c_int, P(C.c_float), c_void_p, c_void_p, c_long, P(C.c_float),
     c_void_p, c_long)
_sig("chase_hip_diag_list_d2s", c_int, c_void_p, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p, c_int)
_sig("chase_hip_convert_d2s", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_convert_s2d", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_diag_d2s", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_axpy_sp", c_int, c_void_p, c_int, c_int, c_int, P(C.c_float), c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_mfma_f64_peak", c_int, c_void_p, P(c_double))
_sig("chase_hip_gemm3m_enabled", c_int)
_sig("chase_hip_host_lapack_warmup", c_int)
_sig("chase_hip_hbm_copy_peak", c_int, c_void_p, c_size_t, P(c_double))
_sig("chase_hip_trsm_left_upper", c_int, c_void_p, c_int, c_char, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_potrf_upper_blocked", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_int)
_sig("chase_hip_hegst_upper", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_long, c_int)
_sig("chase_hip_gev_reduce", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_gev_backtransform", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_trmm_left_upper", c_int, c_void_p, c_int, c_char, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_hegst_product_upper", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_gev_reduce_itype", c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_gev_backtransform_itype", c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_gev_starttransform", c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_gemm_s_op", c_int, *lib.chase_hip_gemm_s.argtypes)
_sig("chase_hip_gemm_c_op", c_int, *lib.chase_hip_gemm_c.argtypes)
_sig("chase_hip_trsm_left_upper_sp", c_int, *lib.chase_hip_trsm_left_upper.argtypes)
_sig("chase_hip_trmm_left_upper_sp", c_int, *lib.chase_hip_trmm_left_upper.argtypes)
_sig("chase_hip_potrf_upper_blocked_sp", c_int, *lib.chase_hip_potrf_upper_blocked.argtypes)
_sig("chase_hip_hegst_upper_sp", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_gev_reduce_sp", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_gev_backtransform_sp", c_int, *lib.chase_hip_gev_backtransform.argtypes)
_sig("chase_hip_gev_starttransform_sp", c_int, *lib.chase_hip_gev_backtransform.argtypes)


def check(code, where):
    if code != 0:
        raise ChaseHipError(code, where, lib.chase_hip_last_error().decode())
    return code


def _z2(x):
    x = complex(x)
    return (c_double * 2)(x.real, x.imag)


def _c2(x):
    x = complex(x)
    return (C.c_float * 2)(x.real, x.imag)


class DeviceArray:
    """A column-major device matrix/vector owned by a Context (any numpy dtype; the kernels take fp64 / complex fp64 and,
    for the mixed-precision filter, fp32 / complex fp32)."""

    def __init__(self, ctx, shape, dtype):
        self.ctx = ctx
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = c_void_p()
        check(lib.chase_hip_malloc(ctx.h, C.byref(p), self.nbytes), "chase_hip_malloc")
        self.ptr = p.value
        ctx._live.append(self)

    @property
    def ld(self):
        return self.shape[0]

    def offset(self, col):
        return self.ptr + col * self.shape[0] * self.dtype.itemsize

    def upload(self, host):
        a = np.asfortranarray(host, dtype=self.dtype)
        assert a.shape == self.shape, (a.shape, self.shape)
        check(lib.chase_hip_memcpy_h2d(self.ctx.h, self.ptr, a.ctypes.data, self.nbytes), "memcpy_h2d")
        return self

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype, order="F")
        check(lib.chase_hip_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, self.nbytes), "memcpy_d2h")
        return out

    def free(self):
        if self.ptr:
            lib.chase_hip_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    def __init__(self, device=0, stream=None):
        h = c_void_p()
        check(lib.chase_hip_ctx_create(C.byref(h), device, stream), "chase_hip_ctx_create")
        self.h = h
        self.device = device
        self._live = []

    def close(self):
        if self.h:
            for a in self._live:
                a.free()
            self._live = []
            lib.chase_hip_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        check(lib.chase_hip_ctx_sync(self.h), "ctx_sync")

    def oplog(self, on):
        """Start (fresh) / stop the operator log of this context (chase_hip_ctx_oplog)."""
        check(lib.chase_hip_ctx_oplog(self.h, int(on)), "ctx_oplog")

    def oplog_lines(self):
        return lib.chase_hip_ctx_oplog_text(self.h).decode().splitlines()

    def info(self):
        ncu, clk, mem = c_int(), c_int(), c_size_t()
        name = C.create_string_buffer(128)
        check(lib.chase_hip_device_info(self.h, C.byref(ncu), C.byref(clk), C.byref(mem), name, 128), "device_info")
        return {"num_cu": ncu.value, "clock_khz": clk.value, "hbm_bytes": mem.value, "name": name.value.decode()}

    def bus_id(self):
        b = C.create_string_buffer(64)
        check(lib.chase_hip_device_bus_id(self.h, b, 64), "device_bus_id")
        return b.value.decode()

    def empty(self, shape, dtype):
        return DeviceArray(self, shape, dtype)

    def array(self, host):
        host = np.asarray(host)
        dt = np.complex128 if np.iscomplexobj(host) else np.float64
        if host.ndim == 1:
            host = host.reshape(-1, 1)
        return DeviceArray(self, host.shape, dt).upload(host)

    def timer_start(self):
        check(lib.chase_hip_timer_start(self.h), "timer_start")

    def timer_stop(self):
        ms = C.c_float()
        check(lib.chase_hip_timer_stop(self.h, C.byref(ms)), "timer_stop")
        return ms.value

    def gemm(self, opA, m, n, k, alpha, A, lda, B, ldb, beta, Cm, ldc, cplx):
        """Raw-pointer GEMM: A, B, Cm are device addresses (ints)."""
        op = opA.encode()[0:1]
        if cplx:
            check(lib.chase_hip_gemm_z(self.h, op, m, n, k, _z2(alpha), A, lda, B, ldb, _z2(beta), Cm, ldc), "gemm_z")
        else:
            check(lib.chase_hip_gemm_d(self.h, op, m, n, k, float(alpha), A, lda, B, ldb, float(beta), Cm, ldc),
                  "gemm_d")

    def gemm32(self, opA, m, n, k, alpha, A, lda, B, ldb, beta, Cm, ldc, cplx, split=False):
        """Single-precision GEMM (fp32 / complex fp32, op(A) = N only): A, B, Cm are device addresses (ints).
        split: the bf16x3 product on the bf16 matrix cores instead of the fp32 MFMA one."""
        op = opA.encode()[0:1]
        if cplx:
            f = lib.chase_hip_gemm_c_bf16x3 if split else lib.chase_hip_gemm_c
            check(f(self.h, op, m, n, k, _c2(alpha), A, lda, B, ldb, _c2(beta), Cm, ldc), "gemm_c")
        else:
            f = lib.chase_hip_gemm_s_bf16x3 if split else lib.chase_hip_gemm_s
            check(f(self.h, op, m, n, k, float(alpha), A, lda, B, ldb, float(beta), Cm, ldc), "gemm_s")

    def gemm32w(self, opA, m, n, k, alpha, A, lda, B, ldb, beta, Cm, ldc, cplx, split=False):
        """fp32 operands, fp64 result and scalars, op(A) = N or C (the grid filter's product): device addresses (ints).
        split: as in gemm32."""
        op = opA.encode()[0:1]
        if cplx:
            f = lib.chase_hip_gemm_cz_bf16x3 if split else lib.chase_hip_gemm_cz
            check(f(self.h, op, m, n, k, _z2(alpha), A, lda, B, ldb, _z2(beta), Cm, ldc), "gemm_cz")
        else:
            f = lib.chase_hip_gemm_sd_bf16x3 if split else lib.chase_hip_gemm_sd
            check(f(self.h, op, m, n, k, float(alpha), A, lda, B, ldb, float(beta), Cm, ldc), "gemm_sd")

    def bf16x3_pack_bytes(self, m, k, cplx):
        """Bytes of the packed bf16x3 image of an m x k operand (chase_hip_bf16x3_pack_bytes)."""
        b = c_size_t()
        check(lib.chase_hip_bf16x3_pack_bytes(int(cplx), m, k, C.byref(b)), "bf16x3_pack_bytes")
        return b.value

    def bf16x3_pack(self, m, k, A, lda, packed, cplx, src_f64=False):
        """packed = the bf16x3 image of the m x k fp32 (src_f64: fp64) matrix at device address A; every byte is written."""
        check(lib.chase_hip_bf16x3_pack(self.h, int(cplx), int(src_f64), m, k, A, lda, packed), "bf16x3_pack")

    def bf16x3_pack_diag(self, n, H64, ldh, packed, cplx):
        """The n diagonal entries of an n x n pack, from the fp64 H; nothing else of packed is written."""
        check(lib.chase_hip_bf16x3_pack_diag(self.h, int(cplx), n, H64, ldh, packed), "bf16x3_pack_diag")

    def gemm32p(self, m, n, k, alpha, packedA, B, ldb, beta, Cm, ldc, cplx):
        """The bf16x3 product of gemm32(..., split=True) with A given as its pack (bf16x3_pack of the same m, k): same bits."""
        if cplx:
            check(lib.chase_hip_gemm_c_bf16x3p(self.h, m, n, k, _c2(alpha), packedA, B, ldb, _c2(beta), Cm, ldc), "gemm_c_bf16x3p")
        else:
            check(lib.chase_hip_gemm_s_bf16x3p(self.h, m, n, k, float(alpha), packedA, B, ldb, float(beta), Cm, ldc),
                  "gemm_s_bf16x3p")

    def set_gemm_min_rounds(self, rounds):
        """chase_hip_ctx_set_gemm_min_rounds: > 0 while products share the chip with a collective (they are cut along K)."""
        check(lib.chase_hip_ctx_set_gemm_min_rounds(self.h, int(rounds)), "ctx_set_gemm_min_rounds")

    def gemm_sp_counters(self, reset=False):
        """(wide_calls, split_calls, pieces) of the gemm32w products of this context (chase_hip_ctx_gemm_sp_counters)."""
        w, s, p = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        check(lib.chase_hip_ctx_gemm_sp_counters(self.h, C.byref(w), C.byref(s), C.byref(p), int(reset)), "ctx_gemm_sp_counters")
        return w.value, s.value, p.value

    def diag_list_d2s(self, H, ldh, Hs, ldhs, rows, cols, cnt, cplx):
        """Hs[rows[i], cols[i]] (fp32) = H[rows[i], cols[i]] (fp64), i < cnt; rows, cols: device addresses of int32 lists."""
        check(lib.chase_hip_diag_list_d2s(self.h, int(cplx), H, ldh, Hs, ldhs, rows, cols, cnt), "diag_list_d2s")

    def convert_d2s(self, m, n, src, ld_src, dst, ld_dst, cplx):
        """dst (fp32) = src (fp64), round to nearest; device addresses, leading dimensions in elements."""
        check(lib.chase_hip_convert_d2s(self.h, int(cplx), m, n, src, ld_src, dst, ld_dst), "convert_d2s")

    def convert_s2d(self, m, n, src, ld_src, dst, ld_dst, cplx):
        """dst (fp64) = src (fp32), exact."""
        check(lib.chase_hip_convert_s2d(self.h, int(cplx), m, n, src, ld_src, dst, ld_dst), "convert_s2d")

    def diag_d2s(self, n, H, ldh, Hs, ldhs, cplx):
        """Hs[i, i] (fp32) = H[i, i] (fp64) for i < n; nothing else of Hs is written."""
        check(lib.chase_hip_diag_d2s(self.h, int(cplx), n, H, ldh, Hs, ldhs), "diag_d2s")

    def axpy_sp(self, m, n, gamma, X, ldx, Y, ldy, cplx):
        """Y_j += gamma X_j on m x n fp32 / complex fp32 columns; device addresses, leading dimensions in elements."""
        check(lib.chase_hip_axpy_sp(self.h, int(cplx), m, n, _c2(gamma), X, ldx, Y, ldy), "axpy_sp")

    def scale_rows_sp(self, m, n, X, ldx, row0, s, cplx):
        """X[row0:m, :n] *= s on fp32 / complex fp32 columns (one fp32 multiply per component); device address, ld in elements."""
        check(lib.chase_hip_scale_rows_sp(self.h, int(cplx), m, n, X, ldx, row0, float(s)), "scale_rows_sp")

    def kconj_sp(self, N, n, first, ldf, second, lds, cplx):
        """second = K-conjugate of first (n fp32 / complex fp32 columns of N rows): halves swapped, complex entries conjugated."""
        check(lib.chase_hip_kconj_sp(self.h, int(cplx), N, n, first, ldf, second, lds), "kconj_sp")

    def to_single(self, dA):
        """fp32 / complex fp32 copy of an fp64 / complex fp64 DeviceArray, converted on the device."""
        cplx = dA.dtype == np.complex128
        out = self.empty(dA.shape, np.complex64 if cplx else np.float32)
        self.convert_d2s(dA.shape[0], dA.shape[1], dA.ptr, dA.ld, out.ptr, out.ld, cplx)
        return out

    def to_double(self, dA):
        """fp64 / complex fp64 copy of an fp32 / complex fp32 DeviceArray, converted on the device."""
        cplx = dA.dtype == np.complex64
        out = self.empty(dA.shape, np.complex128 if cplx else np.float64)
        self.convert_s2d(dA.shape[0], dA.shape[1], dA.ptr, dA.ld, out.ptr, out.ld, cplx)
        return out

    def hash64(self, ptr, m, n, ld, cplx):
        """64-bit content hash of a device matrix (chase_hip_hash64)"""
        h = C.c_ulonglong()
        check(lib.chase_hip_hash64(self.h, int(cplx), m, n, ptr, ld, C.byref(h)), "hash64")
        return h.value

    def gen_clement(self, N, cplx, scale=1.0, perturb=0.0, seed=42):
        """Whole N x N Clement-type test matrix generated in HBM (see chase_hip_gen_clement)."""
        dH = self.empty((N, N), np.complex128 if cplx else np.float64)
        check(lib.chase_hip_gen_clement(self.h, int(cplx), dH.ptr, N, N, N, N, N, 1, 0, 0, N, 1, 0, 0, float(scale),
                                        float(perturb), seed), "gen_clement")
        return dH

    def load_matrix(self, path, N, cplx):
        """Whole N x N matrix from a raw column-major binary file (the reference's input format) into HBM."""
        dH = self.empty((N, N), np.complex128 if cplx else np.float64)
        check(lib.chase_hip_load_matrix_shard(self.h, str(path).encode(), int(cplx), N, N, N, N, 1, 0, N, 1, 0, dH.ptr, N),
              "load_matrix_shard")
        return dH

    def save_matrix(self, path, dA):
        cplx = dA.dtype == np.complex128
        check(lib.chase_hip_save_matrix(self.h, str(path).encode(), int(cplx), dA.shape[0],
                                        dA.shape[1] if len(dA.shape) > 1 else 1, dA.ptr, dA.shape[0]), "save_matrix")

    def gen_bse(self, N, cplx=True, dmin=1.0, dmax=11.0, offdiag=1e-3, seed=7):
        """Whole N x N synthetic Bethe-Salpeter matrix generated in HBM (see chase_hip_gen_bse)."""
        dH = self.empty((N, N), np.complex128 if cplx else np.float64)
        check(lib.chase_hip_gen_bse(self.h, int(cplx), dH.ptr, N, N, N, N, N, 1, 0, N, 1, 0, float(dmin), float(dmax),
                                    float(offdiag), seed), "gen_bse")
        return dH

    def mfma_f64_peak(self):
        t = c_double()
        check(lib.chase_hip_mfma_f64_peak(self.h, C.byref(t)), "mfma_f64_peak")
        return t.value

    def hbm_copy_peak(self, nbytes=1 << 30):
        g = c_double()
        check(lib.chase_hip_hbm_copy_peak(self.h, nbytes, C.byref(g)), "hbm_copy_peak")
        return g.value

    # ---- generalized problem H x = lambda S x (capi_gev.hip); device addresses (ints), leading dimensions in elements ----
    def trsm_left_upper(self, op, n, nrhs, R, ldr, B, ldb, cplx):
        """B <- op(R)^{-1} B, R upper triangular, op 'N' or 'C'"""
        check(lib.chase_hip_trsm_left_upper(self.h, int(cplx), op.encode()[0:1], n, nrhs, R, ldr, B, ldb), "trsm_left_upper")

    def potrf_upper_blocked(self, n, A, lda, cplx, outer_nb=0):
        """In-place upper Cholesky that leaves the strictly lower triangle alone; returns the LAPACK info (0, or the first bad pivot)"""
        info = lib.chase_hip_potrf_upper_blocked(self.h, int(cplx), n, A, lda, outer_nb)
        return info if info >= 0 else check(info, "potrf_upper_blocked")

    def hegst_upper(self, n, A, lda, U, ldu, cplx, nb=0):
        """A <- U^{-H} A U^{-1}, exactly Hermitian, both triangles"""
        check(lib.chase_hip_hegst_upper(self.h, int(cplx), n, A, lda, U, ldu, nb), "hegst_upper")

    def gev_reduce(self, n, A, lda, S, lds, cplx):
        """S <- U (S = U^H U), A <- U^{-H} A U^{-1}; returns 0 or the pivot at which S is not positive definite (A untouched)"""
        info = lib.chase_hip_gev_reduce(self.h, int(cplx), n, A, lda, S, lds)
        return info if info >= 0 else check(info, "gev_reduce")

    def gev_backtransform(self, n, ncols, U, ldu, X, ldx, cplx):
        """X <- U^{-1} X"""
        check(lib.chase_hip_gev_backtransform(self.h, int(cplx), n, ncols, U, ldu, X, ldx), "gev_backtransform")

    def trmm_left_upper(self, op, n, ncols, U, ldu, X, ldx, cplx):
        """X <- op(U) X in place, U upper triangular, op 'N' or 'C'"""
        check(lib.chase_hip_trmm_left_upper(self.h, int(cplx), op.encode()[0:1], n, ncols, U, ldu, X, ldx), "trmm_left_upper")

    def hegst_product_upper(self, n, A, lda, U, ldu, cplx):
        """A <- U A U^H, exactly Hermitian, both triangles"""
        check(lib.chase_hip_hegst_product_upper(self.h, int(cplx), n, A, lda, U, ldu), "hegst_product_upper")

    def gev_reduce_itype(self, itype, factor, n, A, lda, S, lds, cplx):
        """itype 1: A <- U^{-H} A U^{-1}; 2, 3: A <- U A U^H.  factor 1: S <- U first (returns the bad pivot if there is one);
        factor 0: S already holds U"""
        info = lib.chase_hip_gev_reduce_itype(self.h, int(cplx), itype, int(factor), n, A, lda, S, lds)
        return info if info >= 0 else check(info, "gev_reduce_itype")

    def gev_backtransform_itype(self, itype, n, ncols, U, ldu, X, ldx, cplx):
        """X <- U^{-1} X (itype 1, 2) or U^H X (itype 3)"""
        check(lib.chase_hip_gev_backtransform_itype(self.h, int(cplx), itype, n, ncols, U, ldu, X, ldx), "gev_backtransform_itype")

    def gev_starttransform(self, itype, n, ncols, U, ldu, X, ldx, cplx):
        """X <- U X (itype 1, 2) or U^{-H} X (itype 3): the inverse of gev_backtransform_itype"""
        check(lib.chase_hip_gev_starttransform(self.h, int(cplx), itype, n, ncols, U, ldu, X, ldx), "gev_starttransform")

    # ---- the same on fp32 / complex fp32 data, itype 1 (the _sp entry points of capi_gev.hip) ----
    def gemm32op(self, opA, m, n, k, alpha, A, lda, B, ldb, beta, Cm, ldc, cplx):
        """gemm32 with op(A) = N or C (real: T as well); N is gemm32 bit for bit, C is N on the explicit A^H bit for bit"""
        op = opA.encode()[0:1]
        if cplx:
            check(lib.chase_hip_gemm_c_op(self.h, op, m, n, k, _c2(alpha), A, lda, B, ldb, _c2(beta), Cm, ldc), "gemm_c_op")
        else:
            check(lib.chase_hip_gemm_s_op(self.h, op, m, n, k, float(alpha), A, lda, B, ldb, float(beta), Cm, ldc), "gemm_s_op")

    def trsm_left_upper_sp(self, op, n, nrhs, R, ldr, B, ldb, cplx):
        check(lib.chase_hip_trsm_left_upper_sp(self.h, int(cplx), op.encode()[0:1], n, nrhs, R, ldr, B, ldb), "trsm_left_upper_sp")

    def trmm_left_upper_sp(self, op, n, ncols, U, ldu, X, ldx, cplx):
        check(lib.chase_hip_trmm_left_upper_sp(self.h, int(cplx), op.encode()[0:1], n, ncols, U, ldu, X, ldx), "trmm_left_upper_sp")

    def potrf_upper_blocked_sp(self, n, A, lda, cplx, outer_nb=0):
        info = lib.chase_hip_potrf_upper_blocked_sp(self.h, int(cplx), n, A, lda, outer_nb)
        return info if info >= 0 else check(info, "potrf_upper_blocked_sp")

    def hegst_upper_sp(self, n, A, lda, U, ldu, cplx):
        check(lib.chase_hip_hegst_upper_sp(self.h, int(cplx), n, A, lda, U, ldu), "hegst_upper_sp")

    def gev_reduce_sp(self, factor, n, A, lda, S, lds, cplx):
        """factor 1: S <- U, then A <- U^{-H} A U^{-1} (returns the bad pivot if there is one, A untouched); factor 0: S holds U"""
        info = lib.chase_hip_gev_reduce_sp(self.h, int(cplx), int(factor), n, A, lda, S, lds)
        return info if info >= 0 else check(info, "gev_reduce_sp")

    def gev_backtransform_sp(self, n, ncols, U, ldu, X, ldx, cplx):
        check(lib.chase_hip_gev_backtransform_sp(self.h, int(cplx), n, ncols, U, ldu, X, ldx), "gev_backtransform_sp")

    def gev_starttransform_sp(self, n, ncols, U, ldu, X, ldx, cplx):
        check(lib.chase_hip_gev_starttransform_sp(self.h, int(cplx), n, ncols, U, ldu, X, ldx), "gev_starttransform_sp")


# ---- non-GEMM kernels -------------------------------------------------------------------------------------------------
_sig("chase_hip_set_lapack_lib", c_int, C.c_char_p)
_sig("chase_hip_lapack_provider", C.c_char_p)
_sig("chase_hip_set_host_threads", c_int, c_int)
_sig("chase_hip_ctx_set_phase", c_int, c_void_p, c_int)
_sig("chase_hip_ctx_set_gemm_min_rounds", c_int, c_void_p, c_int)
_sig("chase_hip_fill_normal", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_long, c_long, c_long,
     C.c_ulonglong)
_sig("chase_hip_gen_clement", c_int, c_void_p, c_int, c_void_p, c_long, c_int, c_int, c_long, c_int, c_int, c_int,
     c_long, c_int, c_int, c_int, c_long, c_double, c_double, C.c_ulonglong)
_sig("chase_hip_gen_bse", c_int, c_void_p, c_int, c_void_p, c_long, c_int, c_int, c_long, c_int, c_int, c_int, c_int, c_int,
     c_int, c_double, c_double, c_double, C.c_ulonglong)
_sig("chase_hip_load_matrix_shard", c_int, c_void_p, C.c_char_p, c_int, c_long, c_int, c_int, c_int, c_int, c_int, c_int,
     c_int, c_int, c_void_p, c_long)
_sig("chase_hip_save_matrix", c_int, c_void_p, C.c_char_p, c_int, c_int, c_int, c_void_p, c_long)
_sig("chase_hip_shift_diag", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_double)
_sig("chase_hip_shift_list", c_int, c_void_p, c_int, c_void_p, c_long, c_void_p, c_void_p, c_int, c_double)
_sig("chase_hip_lacpy", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_swap_cols", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_long, c_long)
_sig("chase_hip_permute_cols", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_long, P(c_int), P(c_int),
     c_int)
_sig("chase_hip_upload_matrix", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_download_matrix", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_scale_rows", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_int, c_double)
_sig("chase_hip_scale_rows_bc", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_long, c_long, c_int, c_int,
     c_double)
_sig("chase_hip_conj", c_int, c_void_p, c_int, c_int, c_void_p, c_long)
_sig("chase_hip_resid_norms", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p,
     c_void_p, c_int)
_sig("chase_hip_gemm_workspace_bytes", c_size_t, c_int, C.c_char, c_int, c_int, c_int, c_int, c_int)
_sig("chase_hip_herk", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_herkx", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p, c_long, c_int)
_sig("chase_hip_abs_trace", c_int, c_void_p, c_int, c_int, c_void_p, c_long, P(c_double))
_sig("chase_hip_potrf_upper", c_int, c_void_p, c_int, c_int, c_void_p, c_long)
_sig("chase_hip_trsm_right_upper", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_cholqr", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long, c_int, c_long)
_sig("chase_hip_houseqr", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long)
_sig("chase_hip_heevd", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p)
_sig("chase_hip_heevd_gpu", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p)
_sig("chase_hip_heevd_host", c_int, c_int, c_int, c_void_p, c_long, c_void_p)
_sig("chase_hip_stedc", c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_long)
_sig("chase_hip_stemr_host", c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int)
_sig("chase_hip_col_dot", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p)
_sig("chase_hip_col_nrm2", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p)
_sig("chase_hip_col_axpy", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_double, c_void_p, c_long,
     c_void_p, c_long)
_sig("chase_hip_col_scal", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_long)
_sig("chase_hip_col_sumsq", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p)
_sig("chase_hip_sqrt_inplace", c_int, c_void_p, c_void_p, c_int)
_sig("chase_hip_fill_normal_bc", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_long, c_int, c_int, c_int,
     C.c_ulonglong)
_sig("chase_hip_rows_indexed", c_int, c_void_p, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p, c_int, c_int, c_int)
# kernels of the single-precision solver
_sig("chase_hip_shift_diag_sp", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_double)
_sig("chase_hip_resid_norms_sp", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p, c_void_p)
_sig("chase_hip_lacpy_sp", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_scale_rows_sp", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_int, C.c_float)
_sig("chase_hip_kconj_sp", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_swap_cols_sp", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_long, c_long)
_sig("chase_hip_permute_cols_sp", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_long, P(c_int), P(c_int), c_int)
_sig("chase_hip_upload_matrix_sp", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_download_matrix_sp", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long)
_sig("chase_hip_complete_hermitian_sp", c_int, c_void_p, c_int, c_char, c_int, c_void_p, c_long)
_sig("chase_hip_pack_upper", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p)
_sig("chase_hip_unpack_upper", c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_long, c_int)


# ---- host solver (include/chase_hip_solver.h) ------------------------------------------------------------------------
class Stats(C.Structure):
    _fields_ = [("iterations", c_size_t), ("filtered_vecs", c_size_t), ("lanczos_vecs", c_size_t),
                ("locked", c_size_t), ("t_all", c_double), ("t_init", c_double), ("t_lanczos", c_double),
                ("t_filter", c_double), ("t_qr", c_double), ("t_rr", c_double), ("t_resid", c_double),
                ("filter_ms_device", c_double), ("lowerb", c_double), ("upperb", c_double), ("lambda_", c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_sig("chase_hip_solver_create", c_int, P(c_void_p), c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_void_p, c_size_t,
     c_void_p, c_size_t, c_void_p, c_int)
_sig("chase_hip_solver_destroy", c_int, c_void_p)
_sig("chase_hip_solver_set", c_int, c_void_p, C.c_char_p, c_double)
_sig("chase_hip_solver_get", c_int, c_void_p, C.c_char_p, P(c_double))
_sig("chase_hip_solver_solve", c_int, c_void_p, c_int)
ITER_FN = C.CFUNCTYPE(c_int, c_void_p, c_size_t, c_size_t, c_size_t, c_size_t)
_sig("chase_hip_solver_set_iteration_hook", c_int, c_void_p, ITER_FN, c_void_p)
_sig("chase_hip_set_gemm3m", c_int, c_int)
_sig("chase_hip_ctx_gemm_counters", c_int, c_void_p, c_int, P(c_double), P(c_double), P(C.c_ulonglong), c_int)
_sig("chase_hip_solver_stats", c_int, c_void_p, P(Stats))
_sig("chase_hip_solver_resid", P(c_double), c_void_p)
_sig("chase_hip_solver_trace", C.c_char_p, c_void_p)
_sig("chase_hip_solver_recompute_residuals", c_int, c_void_p, c_size_t, c_void_p, c_void_p)
_sig("chase_hip_solver_tape_mode", c_int, c_void_p, c_int)
_sig("chase_hip_solver_tape_data", c_int, c_void_p, P(P(c_double)), P(c_size_t))
_sig("chase_hip_solver_tape_load", c_int, c_void_p, c_void_p, c_size_t)
_sig("chase_hip_resid_norms_dev", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p,
     c_void_p, c_int)
_sig("chase_hip_solver_peek_v", c_int, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("chase_hip_solver_hash_v", c_int, c_void_p, c_void_p, c_size_t, P(C.c_ulonglong))
_sig("chase_hip_op_start", c_int, c_void_p)
_sig("chase_hip_op_end", c_int, c_void_p)
_sig("chase_hip_op_initvecs", c_int, c_void_p, c_int)
_sig("chase_hip_op_reinit_columns", c_int, c_void_p, c_size_t, P(c_size_t), c_size_t)
_sig("chase_hip_op_shift", c_int, c_void_p, c_double, c_int)
_sig("chase_hip_op_filter_phase", c_int, c_void_p, c_int)
_sig("chase_hip_op_hemm", c_int, c_void_p, c_size_t, P(c_double), P(c_double), c_size_t, c_size_t)
_sig("chase_hip_op_qr", c_int, c_void_p, c_size_t, c_double)
_sig("chase_hip_op_rr", c_int, c_void_p, c_void_p, c_size_t)
_sig("chase_hip_op_resd", c_int, c_void_p, c_void_p, c_void_p, c_size_t)
_sig("chase_hip_op_swap", c_int, c_void_p, c_size_t, c_size_t)
_sig("chase_hip_op_lock", c_int, c_void_p, c_size_t)
_sig("chase_hip_op_lanczos", c_int, c_void_p, c_size_t, c_size_t, P(c_double), c_void_p, c_void_p, c_void_p)
_sig("chase_hip_op_lanczos_dos", c_int, c_void_p, c_size_t, c_size_t, c_void_p)
_sig("chase_hip_op_check_symmetry", c_int, c_void_p, P(c_int))
_sig("chase_hip_op_sym_or_herm", c_int, c_void_p, c_char)
_sig("chase_hip_complete_hermitian", c_int, c_void_p, c_int, c_char, c_int, c_void_p, c_long)
_sig("chase_hip_hash64", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, P(C.c_ulonglong))
_sig("chase_hip_cols_indexed", c_int, c_void_p, c_int, c_int, c_void_p, c_long, c_void_p, c_long, c_void_p, c_int)
_sig("chase_hip_tri_mask_bc", c_int, c_void_p, c_int, c_char, c_int, c_int, c_void_p, c_long, c_long, c_int, c_int, c_long, c_int,
     c_int)
_sig("chase_hip_conj_transpose_add", c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_long, c_void_p, c_void_p, c_void_p, c_long)


def set_iteration_hook(solver, fn):
    """Installs fn(iteration, filtered_vecs, locked, unconverged) as the outer-iteration observer of a solver object."""
    if fn is None:
        solver._iter_cb = ITER_FN()
    else:
        def _cb(user, it, filtered, locked, unconverged):
            try:
                return 1 if fn(int(it), int(filtered), int(locked), int(unconverged)) else 0
            except Exception as e:  # pragma: no cover - never unwind through the C++ driver
                print("iteration hook failed:", repr(e), flush=True)
                return 1
        solver._iter_cb = ITER_FN(_cb)                 # keep the thunk alive
    check(lib.chase_hip_solver_set_iteration_hook(solver.h, solver._iter_cb, None), "set_iteration_hook")


def recompute_residuals(solver, ncols, lam=None):
    """|| H v_j - lambda_j v_j || for the first ncols vectors of a solver object, from a fresh four-product H V."""
    lam = np.ascontiguousarray(solver.ritzv[:ncols] if lam is None else lam, dtype=np.float64)
    out = np.zeros(ncols)
    check(lib.chase_hip_solver_recompute_residuals(solver.h, ncols, lam.ctypes.data, out.ctypes.data), "recompute_residuals")
    return out


TAPE_OFF, TAPE_RECORD, TAPE_REPLAY = 0, 1, 2


def tape_mode(solver, mode):
    """0 off, 1: the next solves record everything the Impl tells the driver, 2: they replay the loaded tape (tape.hpp)."""
    check(lib.chase_hip_solver_tape_mode(solver.h, int(mode)), "tape_mode")


def tape_get(solver):
    """The scalar tape of the last recorded solve as a float64 array (frames: tag, count, values...)."""
    p, n = P(c_double)(), c_size_t()
    check(lib.chase_hip_solver_tape_data(solver.h, C.byref(p), C.byref(n)), "tape_data")
    return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0)


def tape_load(solver, tape):
    t = np.ascontiguousarray(tape, dtype=np.float64)
    check(lib.chase_hip_solver_tape_load(solver.h, t.ctypes.data, t.size), "tape_load")


def gemm_counters(ctx, phase, reset=False):
    """(model flops, executed flops, products) of the GEMMs a context issued in `phase` (1 = Chebyshev filter)."""
    a, b, n = c_double(), c_double(), C.c_ulonglong()
    check(lib.chase_hip_ctx_gemm_counters(ctx.h, phase, C.byref(a), C.byref(b), C.byref(n), int(reset)), "gemm_counters")
    return a.value, b.value, n.value


class GemmLaunch(C.Structure):
    """One launch of a product (chase_hip_gemm_launch)."""
    _fields_ = [(f, c_int) for f in ("row0", "col0", "k0", "m", "n", "k", "beta_one", "bn_cols", "narrow", "m3", "ragged",
                                     "glds_ok", "gm", "gn")] + \
               [("full_tiles", c_long), ("tail_tiles", c_long)] + \
               [(f, c_int) for f in ("tail_sk", "tail_kchunk", "group_rows", "forced_split")] + \
               [("slab_bytes", c_size_t), ("plane_bytes", c_size_t)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_sig("chase_hip_gemm_plan", c_int, c_int, c_char, c_int, c_int, c_int, c_long, c_long, c_int, c_int, c_int, c_int,
     P(GemmLaunch), c_int)


def gemm_plan(cplx, op, m, n, k, lda=None, ldb=None, aligned=True, phase=0, num_cu=256, min_rounds=0):
    """The launches chase_hip_gemm_{d,z} makes for this product, as dicts (chase_hip_gemm_plan; host-only).  lda / ldb default
    to the tightest leading dimensions."""
    lda = (m if op == "N" else k) if lda is None else lda
    ldb = k if ldb is None else ldb
    args = (int(cplx), op.encode(), m, n, k, max(lda, 1), max(ldb, 1), int(aligned), phase, num_cu, min_rounds)
    cnt = lib.chase_hip_gemm_plan(*args, None, 0)
    if cnt < 0:
        check(cnt, "gemm_plan")
    out = (GemmLaunch * max(cnt, 1))()
    assert lib.chase_hip_gemm_plan(*args, out, cnt) == cnt
    return [out[i].as_dict() for i in range(cnt)]


class GemmSpLaunch(C.Structure):
    """chase_hip_gemm_sp_launch (include/chase_hip.h)"""
    _fields_ = [(n, c_int) for n in ("bn", "gm", "gn", "sk", "kchunk", "min_piece_k")] + [("slab_bytes", c_size_t)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_sig("chase_hip_gemm_sp_plan", c_int, c_int, c_int, c_char, c_int, c_int, c_int, c_int, c_int, P(GemmSpLaunch))
_sig("chase_hip_gemm_sp_workspace_bytes", c_size_t, c_int, c_int, c_char, c_int, c_int, c_int, c_int, c_int)
_sig("chase_hip_ctx_gemm_sp_counters", c_int, c_void_p, P(C.c_ulonglong), P(C.c_ulonglong), P(C.c_ulonglong), c_int)


def gemm_sp_plan(cplx, op, m, n, k, split=False, num_cu=256, min_rounds=0):
    """The launch chase_hip_gemm_sd / _cz (split: their bf16x3 twins) make for this product while the context's gemm_min_rounds
    is min_rounds, as a dict (chase_hip_gemm_sp_plan; host-only): tiles, K pieces and their workspace."""
    out = GemmSpLaunch()
    check(lib.chase_hip_gemm_sp_plan(int(split), int(cplx), op.encode(), m, n, k, num_cu, min_rounds, C.byref(out)), "gemm_sp_plan")
    return out.as_dict()


def gemm_sp_workspace_bytes(cplx, op, m, n, k, split=False, num_cu=256, min_rounds=0):
    return lib.chase_hip_gemm_sp_workspace_bytes(int(split), int(cplx), op.encode(), m, n, k, num_cu, min_rounds)


class Solver:
    """ChaseHip<T> behind the C ABI: the reference's ChASEGPU constructor contract (host H, V, ritzv owned by the
    caller; chase_gpu.hpp:107) plus chase::Solve."""

    def __init__(self, ctx, H, nev, nex, V=None, h_on_device_ptr=None, N=None, cplx=None):
        self.ctx = ctx
        if h_on_device_ptr is None:
            assert H.flags.f_contiguous and H.ndim == 2 and H.shape[0] == H.shape[1]
            self.cplx = bool(np.iscomplexobj(H))
            self.N = H.shape[0]
            self.H = H
            hptr, on_dev = H.ctypes.data, 0
        else:
            self.cplx, self.N, self.H = bool(cplx), int(N), None
            hptr, on_dev = h_on_device_ptr, 1
        self.nev, self.nex = nev, nex
        dt = np.complex128 if self.cplx else np.float64
        self.V = np.zeros((self.N, nev + nex), dtype=dt, order="F") if V is None else V
        assert self.V.flags.f_contiguous and self.V.dtype == dt
        self.ritzv = np.zeros(nev + nex, dtype=np.float64)
        h = c_void_p()
        check(lib.chase_hip_solver_create(C.byref(h), ctx.h, int(self.cplx), self.N, nev, nex, hptr, self.N,
                                          self.V.ctypes.data, self.N, self.ritzv.ctypes.data, on_dev),
              "solver_create")
        self.h = h

    def close(self):
        if self.h:
            lib.chase_hip_solver_destroy(self.h)
            self.h = None

    def set(self, **kw):
        for k, v in kw.items():
            check(lib.chase_hip_solver_set(self.h, k.encode(), float(v)), f"solver_set({k})")

    def get(self, key):
        v = c_double()
        check(lib.chase_hip_solver_get(self.h, key.encode(), C.byref(v)), f"solver_get({key})")
        return v.value

    def solve(self, trace=False):
        check(lib.chase_hip_solver_solve(self.h, int(trace)), "solver_solve")
        return self.stats()

    def set_iteration_hook(self, fn):
        """fn(iteration, filtered_vecs, locked, unconverged) -> truthy to leave the iteration loop; None removes it."""
        set_iteration_hook(self, fn)

    def stats(self):
        s = Stats()
        check(lib.chase_hip_solver_stats(self.h, C.byref(s)), "solver_stats")
        return s.as_dict()

    def resid(self):
        p = lib.chase_hip_solver_resid(self.h)
        return np.ctypeslib.as_array(p, shape=(self.nev + self.nex,)).copy()

    def trace(self):
        return lib.chase_hip_solver_trace(self.h).decode().splitlines()

    def recompute_residuals(self, ncols, lam=None):
        return recompute_residuals(self, ncols, lam)

    def peek_v(self):
        out = np.empty_like(self.V, order="F")
        check(lib.chase_hip_solver_peek_v(self.h, self.ctx.h, out.ctypes.data, self.N), "peek_v")
        return out

    # ChaseBase virtuals
    def Start(self): check(lib.chase_hip_op_start(self.h), "Start")
    def End(self): check(lib.chase_hip_op_end(self.h), "End")
    def initVecs(self, random): check(lib.chase_hip_op_initvecs(self.h, int(random)), "initVecs")

    def ReinitColumns(self, fixednev, cols):
        a = (c_size_t * len(cols))(*cols)
        check(lib.chase_hip_op_reinit_columns(self.h, fixednev, a, len(cols)), "ReinitColumns")
    def Shift(self, c, isunshift=False): check(lib.chase_hip_op_shift(self.h, float(c), int(isunshift)), "Shift")
    def FilterPhaseStart(self): check(lib.chase_hip_op_filter_phase(self.h, 1), "FilterPhaseStart")
    def FilterPhaseEnd(self): check(lib.chase_hip_op_filter_phase(self.h, 0), "FilterPhaseEnd")

    def HEMM(self, block, alpha, beta, offset_left, offset_right=0):
        check(lib.chase_hip_op_hemm(self.h, block, _z2(alpha), _z2(beta), offset_left, offset_right), "HEMM")

    def QR(self, fixednev, cond): check(lib.chase_hip_op_qr(self.h, fixednev, float(cond)), "QR")

    def RR(self, block, offset):
        """ritz values are written to self.ritzv[offset:offset+block] (the driver passes GetRitzv()+locked)."""
        check(lib.chase_hip_op_rr(self.h, self.ritzv.ctypes.data + 8 * offset, block), "RR")

    def Resd(self, offset):
        n = self.nev + self.nex - offset
        out = np.zeros(n)
        check(lib.chase_hip_op_resd(self.h, self.ritzv.ctypes.data + 8 * offset, out.ctypes.data, offset), "Resd")
        return out

    def Swap(self, i, j): check(lib.chase_hip_op_swap(self.h, i, j), "Swap")
    def Lock(self, n): check(lib.chase_hip_op_lock(self.h, n), "Lock")

    def Lanczos(self, M, numvec):
        ub = c_double()
        if numvec == 0:
            check(lib.chase_hip_op_lanczos(self.h, M, 0, C.byref(ub), None, None, None), "Lanczos")
            return ub.value
        theta, tau, ritzV = np.zeros(M * numvec), np.zeros(M * numvec), np.zeros(M * M)
        check(lib.chase_hip_op_lanczos(self.h, M, numvec, C.byref(ub), theta.ctypes.data, tau.ctypes.data,
                                       ritzV.ctypes.data), "Lanczos")
        return ub.value, theta, tau, ritzV.reshape(M, M, order="F")

    def checkSymmetryEasy(self):
        f = c_int()
        check(lib.chase_hip_op_check_symmetry(self.h, C.byref(f)), "checkSymmetryEasy")
        return bool(f.value)

    def symOrHermMatrix(self, uplo):
        check(lib.chase_hip_op_sym_or_herm(self.h, uplo.encode()[0:1]), "symOrHermMatrix")


class GevSolver:
    """The lowest nev pairs of a generalized Hermitian-definite problem (fp64, one GPU): itype 1, H x = lambda S x (the default);
    itype 2, H S x = lambda x; itype 3, S H x = lambda x.  H and S (Fortran order, S positive definite; the upper triangles are
    what is read) are uploaded and reduced in place on the device: S = U^H U, C = U^{-H} H U^{-1} (itype 1) or U H U^H (itype 2
    and 3); an ordinary Solver then works on C where it lies (self.solver).  While this object lives the device holds C and U,
    2 N^2 elements.  set / get / solve / stats / resid are the Solver's; eigenpairs() gives the Ritz values and the
    back-transformed vectors, X = U^{-1} Y with X^H S X = I for itype 1 and 2, X = U^H Y with X^H S^{-1} X = I for itype 3.
    update(H, S) moves on to the next pencil of a sequence with the previous vectors as the start block.  S not positive
    definite: ChaseHipError whose code (and .pivot) is the index of the first non-positive pivot."""

    def __init__(self, ctx, H, S, nev, nex, itype=1):
        assert H.ndim == 2 and H.shape[0] == H.shape[1] and S.shape == H.shape
        if itype not in (1, 2, 3):
            raise ValueError("itype must be 1, 2 or 3")
        self.ctx, self.itype = ctx, itype
        self.cplx = bool(np.iscomplexobj(H) or np.iscomplexobj(S))
        self.N, self.nev, self.nex = H.shape[0], nev, nex
        self.H, self.S = H, S                              # the originals, for gev_residuals()
        self.dC, self.dU = self._dev(H), self._dev(S)
        self.solver = None
        info = self._reduce(1, first=True)
        if info > 0:
            self.close()
            raise self._pivot_error(info)
        self.solver = self._solver_class(ctx, None, nev, nex, h_on_device_ptr=self.dC.ptr, N=self.N, cplx=self.cplx)

    @staticmethod
    def _pivot_error(info):
        err = ChaseHipError(info, "gev_reduce", f"S is not positive definite: pivot {info} is not positive")
        err.pivot = info
        return err

    # ---- what depends on the precision (SpGevSolver overrides these) ----
    _solver_class = Solver

    def _dt(self):
        return np.complex128 if self.cplx else np.float64

    def _accepts(self, A):
        """whether a host matrix may be given as H or S: anything that converts to the fp64 type exactly"""
        return bool(np.iscomplexobj(A)) <= self.cplx

    def _dev(self, A):
        """a device copy of a host array in this solver's type"""
        return self.ctx.empty(A.shape, self._dt()).upload(A)

    def _reduce(self, factor, first=False):
        """dC <- its reduction with dU (factor 1: dU <- U first); the constructor's call at itype 1 is the plain entry point"""
        a = (self.N, self.dC.ptr, self.N, self.dU.ptr, self.N, self.cplx)
        return self.ctx.gev_reduce(*a) if first and self.itype == 1 else self.ctx.gev_reduce_itype(self.itype, factor, *a)

    def _backtransform(self, dX, ncols, plain=False):
        """plain: the itype-free entry point (eigenpairs() at itype 1)"""
        a = (self.N, ncols, self.dU.ptr, self.N, dX.ptr, self.N, self.cplx)
        if plain and self.itype == 1:
            self.ctx.gev_backtransform(*a)
        else:
            self.ctx.gev_backtransform_itype(self.itype, *a)

    def _starttransform(self, dX, ncols):
        self.ctx.gev_starttransform(self.itype, self.N, ncols, self.dU.ptr, self.N, dX.ptr, self.N, self.cplx)

    def _residual_products(self, products):
        """dW <- dA dB for every (dA, dB, dW), dA N x N: fresh four-multiplication fp64 products (phase 3)"""
        try:
            check(lib.chase_hip_ctx_set_phase(self.ctx.h, 3), "set_phase")
            for dA, dB, dW in products:
                self.ctx.gemm("N", self.N, dB.shape[1], self.N, 1.0, dA.ptr, self.N, dB.ptr, self.N, 0.0, dW.ptr, self.N, self.cplx)
        finally:
            lib.chase_hip_ctx_set_phase(self.ctx.h, 0)

    def close(self):
        if self.solver:
            self.solver.close()
            self.solver = None
        for d in (self.dC, self.dU):
            if d is not None:
                d.free()
        self.dC = self.dU = None

    def set(self, **kw): self.solver.set(**kw)
    def get(self, key): return self.solver.get(key)
    def solve(self, trace=False): return self.solver.solve(trace)
    def stats(self): return self.solver.stats()
    def resid(self): return self.solver.resid()

    @property
    def ritzv(self):
        return self.solver.ritzv

    def reduced(self):
        """the reduced matrix C as it lies on the device"""
        return self.dC.download()

    def factor(self):
        """U in the upper triangle (below it: what S held)"""
        return self.dU.download()

    def start_vectors(self):
        """the start block (N x (nev + nex)) the next solve() reads when approx is set: after a solve the solver's vectors, after
        update(H, S) their start transform with the new factor"""
        return self.solver.V.copy(order="F")

    def update(self, H, S=None):
        """The next pencil of a sequence; the next solve() starts from the previous vectors (approx = 1, ritzv kept).
        S given: all nev + nex columns of the block are back-transformed with the old factor, S and H are uploaded and reduced,
        and the block is start-transformed with the new factor - all on the device.  S = None: the overlap matrix did not change;
        only H is uploaded and reduced with the stored factor (no Cholesky), and the block stays as it is."""
        assert H.shape == (self.N, self.N) and self._accepts(H)
        nc = self.nev + self.nex
        if S is None:
            self.dC.upload(H)
            self._reduce(0)
        else:
            assert S.shape == H.shape and self._accepts(S)
            dX = self._dev(self.solver.V)
            try:
                self._backtransform(dX, nc)
                self.dU.upload(S)
                self.dC.upload(H)
                info = self._reduce(1)
                if info > 0:
                    raise self._pivot_error(info)
                self._starttransform(dX, nc)
                self.solver.V[...] = dX.download()
            finally:
                dX.free()
            self.S = S
        self.H = H
        self.solver.set(approx=1)

    def eigenpairs(self):
        """(lambda[:nev], X[:, :nev]): itype 1, H X = S X diag(lambda) and X^H S X = I; itype 2, H S X = X diag(lambda) and
        X^H S X = I; itype 3, S H X = X diag(lambda) and X^H S^{-1} X = I.  lambda is fp64, X of the solver's type."""
        dX = self._dev(self.solver.V[:, :self.nev])
        self._backtransform(dX, self.nev, plain=True)
        X = dX.download()
        dX.free()
        return self.solver.ritzv[:self.nev].copy(), X

    def gev_residuals(self):
        """|| H x_j - lambda_j S x_j ||_2 (itype 1), || H S x_j - lambda_j x_j ||_2 (itype 2) or || S H x_j - lambda_j x_j ||_2
        (itype 3), j < nev, in fp64 from fresh products (_residual_products) with the ORIGINAL H and S, which are uploaded again
        for this (two more N^2 blocks while it runs)"""
        lam, X = self.eigenpairs()
        n, k = self.N, self.nev
        full = lambda A: np.triu(A) + np.triu(A, 1).conj().T          # the triangle the reduction read
        dH, dS, dX = self._dev(full(self.H)), self._dev(full(self.S)), self._dev(X)
        dt64 = np.complex128 if self.cplx else np.float64
        dW, dV = self.ctx.empty((n, k), dt64), self.ctx.empty((n, k), dt64)
        out = np.zeros(k)
        try:
            if self.itype == 1:
                self._residual_products([(dH, dX, dW), (dS, dX, dV)])
                rhs = dV
            else:
                first, second = (dS, dH) if self.itype == 2 else (dH, dS)
                self._residual_products([(first, dX, dV), (second, dV, dW)])
                rhs = dX
            check(lib.chase_hip_resid_norms(self.ctx.h, int(self.cplx), n, k, dW.ptr, n, rhs.ptr, n, lam.ctypes.data,
                                            out.ctypes.data, 0), "resid_norms")
        finally:
            for d in (dH, dS, dX, dW, dV):
                d.free()
        return out


_sig("chase_hip_solver_create_sp", c_int, P(c_void_p), c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_void_p, c_size_t,
     c_void_p, c_size_t, c_void_p, c_int)


class SpSolver(Solver):
    """ChaseHipSp<T>: the single-precision Hermitian solver.  H32 (float32 / complex64, Fortran order) and V stay fp32 on the
    device from start to end; ritzv, residuals and every driver scalar are fp64.  Starts with the reference's float defaults (tol
    1e-5, deg 10, maxdeg 18, lanczositer 12).  h_on_device_ptr with N, cplx and ldh: the fp32 matrix already lives in HBM and is
    used in place.  peek_v() returns the block widened to fp64."""

    def __init__(self, ctx, H32, nev, nex, V=None, h_on_device_ptr=None, N=None, cplx=None, ldh=None):
        self.ctx = ctx
        if h_on_device_ptr is None:
            assert H32.flags.f_contiguous and H32.ndim == 2 and H32.shape[0] == H32.shape[1]
            assert H32.dtype in (np.float32, np.complex64), "SpSolver takes an fp32 matrix: round it yourself"
            self.cplx = H32.dtype == np.complex64
            self.N = H32.shape[0]
            self.H = H32
            hptr, on_dev, ldh = H32.ctypes.data, 0, self.N
        else:
            self.cplx, self.N, self.H = bool(cplx), int(N), None
            hptr, on_dev, ldh = h_on_device_ptr, 1, int(ldh or N)
        self.nev, self.nex = nev, nex
        dt = np.complex64 if self.cplx else np.float32
        self.V = np.zeros((self.N, nev + nex), dtype=dt, order="F") if V is None else V
        assert self.V.flags.f_contiguous and self.V.dtype == dt
        self.ritzv = np.zeros(nev + nex, dtype=np.float64)
        h = c_void_p()
        check(lib.chase_hip_solver_create_sp(C.byref(h), ctx.h, int(self.cplx), self.N, nev, nex, hptr, ldh,
                                             self.V.ctypes.data, self.N, self.ritzv.ctypes.data, on_dev), "solver_create_sp")
        self.h = h

    def peek_v(self):
        out = np.empty((self.N, self.nev + self.nex), dtype=np.complex128 if self.cplx else np.float64, order="F")
        check(lib.chase_hip_solver_peek_v(self.h, self.ctx.h, out.ctypes.data, self.N), "peek_v")
        return out


class SpGevSolver(GevSolver):
    """GevSolver at itype 1 on fp32 data: the lowest nev pairs of H x = lambda S x for H32, S32 float32 / complex64 (Fortran order,
    S positive definite; the upper triangles are what is read).  Both are uploaded as they are and reduced in place on the device
    by the fp32 drivers (S = U^H U, C = U^{-H} H U^{-1}); an SpSolver then works on C where it lies (self.solver).  While this
    object lives the device holds C and U, 2 N^2 fp32 elements: no fp64 copy of H, S or C is ever made.  The surface is
    GevSolver's; ritzv and residuals are fp64, the vectors fp32.  S not positive definite: ChaseHipError with .pivot."""

    def __init__(self, ctx, H32, S32, nev, nex):
        assert self._is_fp32(H32) and self._is_fp32(S32), "SpGevSolver takes fp32 matrices: round them yourself"
        super().__init__(ctx, H32, S32, nev, nex)

    _solver_class = SpSolver

    @staticmethod
    def _is_fp32(A):
        return A.dtype in (np.float32, np.complex64)

    def _dt(self):
        return np.complex64 if self.cplx else np.float32

    def _accepts(self, A):
        return self._is_fp32(A) and super()._accepts(A)

    def _reduce(self, factor, first=False):
        return self.ctx.gev_reduce_sp(factor, self.N, self.dC.ptr, self.N, self.dU.ptr, self.N, self.cplx)

    def _backtransform(self, dX, ncols, plain=False):
        self.ctx.gev_backtransform_sp(self.N, ncols, self.dU.ptr, self.N, dX.ptr, self.N, self.cplx)

    def _starttransform(self, dX, ncols):
        self.ctx.gev_starttransform_sp(self.N, ncols, self.dU.ptr, self.N, dX.ptr, self.N, self.cplx)

    def _residual_products(self, products):
        """products with fp32 operands and an fp64 result"""
        for dA, dB, dW in products:
            self.ctx.gemm32w("N", self.N, dB.shape[1], self.N, 1.0, dA.ptr, self.N, dB.ptr, self.N, 0.0, dW.ptr, self.N, self.cplx)


_sig("chase_hip_solver_create_pseudo", c_int, P(c_void_p), c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_void_p,
     c_size_t, c_void_p, c_size_t, c_void_p, c_int)
_sig("chase_hip_op_hemm_h2", c_int, c_void_p, c_size_t, P(c_double), P(c_double), P(c_double), c_size_t, c_size_t)
_sig("chase_hip_op_kconj", c_int, c_void_p, c_size_t)
_sig("chase_hip_pseudo_rr_small", c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p)
_sig("chase_hip_set_identity", c_int, c_void_p, c_int, c_int, c_void_p, c_long)


_sig("chase_hip_solver_lanczos_for_h2", c_int, c_void_p, c_int, c_int, P(c_double), P(c_size_t))


class PseudoSolver(Solver):
    """ChaseHipPseudo<T>: pseudo-Hermitian (BSE) Impl — subspace of 2*(nev+nex) columns, chase::Solve_pseudo."""

    def __init__(self, ctx, H, nev, nex, h_on_device_ptr=None, N=None, cplx=None):
        """H: the host matrix, or None with h_on_device_ptr, N and cplx: the matrix already lives in HBM and is used in place."""
        self.ctx, self.H = ctx, H
        if h_on_device_ptr is None:
            assert H.flags.f_contiguous and H.shape[0] == H.shape[1]
            self.cplx, self.N = bool(np.iscomplexobj(H)), H.shape[0]
            hptr, on_dev = H.ctypes.data, 0
        else:
            self.cplx, self.N = bool(cplx), int(N)
            hptr, on_dev = h_on_device_ptr, 1
        self.nev, self.nex = nev, nex
        dt = np.complex128 if self.cplx else np.float64
        self.ncol = 2 * (nev + nex)
        self.V = np.zeros((self.N, self.ncol), dtype=dt, order="F")
        self.ritzv = np.zeros(self.ncol)
        h = c_void_p()
        check(lib.chase_hip_solver_create_pseudo(C.byref(h), ctx.h, int(self.cplx), self.N, nev, nex, hptr,
                                                 self.N, self.V.ctypes.data, self.N, self.ritzv.ctypes.data, on_dev),
              "solver_create_pseudo")
        self.h = h

    def resid(self):
        p = lib.chase_hip_solver_resid(self.h)
        return np.ctypeslib.as_array(p, shape=(self.ncol,)).copy()

    def HEMM_H2(self, block, alpha, beta, gamma, offset_left, offset_right=0):
        check(lib.chase_hip_op_hemm_h2(self.h, block, _z2(alpha), _z2(beta), _z2(gamma), offset_left, offset_right),
              "HEMM_H2")

    def ApplyKconjugate(self, block):
        check(lib.chase_hip_op_kconj(self.h, block), "ApplyKconjugate")

    def lanczos_for_H2(self, numvec, m):
        ub, idx = c_double(), c_size_t()
        check(lib.chase_hip_solver_lanczos_for_h2(self.h, numvec, m, C.byref(ub), C.byref(idx)), "lanczos_for_H2")
        return ub.value, idx.value

    def RR(self, block, offset):
        check(lib.chase_hip_op_rr(self.h, self.ritzv.ctypes.data + 8 * offset, block), "RR")

    def Resd(self, offset):
        n = self.nev + self.nex - offset
        out = np.zeros(n)
        check(lib.chase_hip_op_resd(self.h, self.ritzv.ctypes.data + 8 * offset, out.ctypes.data, offset), "Resd")
        return out


_sig("chase_hip_solver_create_pseudo_sp", c_int, P(c_void_p), c_void_p, c_int, c_size_t, c_size_t, c_size_t, c_void_p,
     c_size_t, c_void_p, c_size_t, c_void_p, c_int)


class SpPseudoSolver(PseudoSolver):
    """ChaseHipSpPseudo<T>: the single-precision pseudo-Hermitian (BSE) solver.  H32 (float32 / complex64, Fortran order) and V
    (N x 2*(nev+nex)) stay fp32 on the device from start to end; ritzv and resid() are fp64 of length 2*(nev+nex).  Starts with the
    reference's float defaults.  h_on_device_ptr with N, cplx and ldh: the fp32 matrix already lives in HBM and is used in place.
    peek_v() returns the block widened to fp64.  The op methods are PseudoSolver's."""

    def __init__(self, ctx, H32, nev, nex, h_on_device_ptr=None, N=None, cplx=None, ldh=None):
        self.ctx, self.H = ctx, H32
        if h_on_device_ptr is None:
            assert H32.flags.f_contiguous and H32.ndim == 2 and H32.shape[0] == H32.shape[1]
            assert H32.dtype in (np.float32, np.complex64), "SpPseudoSolver takes an fp32 matrix: round it yourself"
            self.cplx, self.N = H32.dtype == np.complex64, H32.shape[0]
            hptr, on_dev, ldh = H32.ctypes.data, 0, self.N
        else:
            self.cplx, self.N = bool(cplx), int(N)
            hptr, on_dev, ldh = h_on_device_ptr, 1, int(ldh or N)
        self.nev, self.nex = nev, nex
        self.ncol = 2 * (nev + nex)
        self.V = np.zeros((self.N, self.ncol), dtype=np.complex64 if self.cplx else np.float32, order="F")
        self.ritzv = np.zeros(self.ncol)
        h = c_void_p()
        check(lib.chase_hip_solver_create_pseudo_sp(C.byref(h), ctx.h, int(self.cplx), self.N, nev, nex, hptr, ldh,
                                                    self.V.ctypes.data, self.N, self.ritzv.ctypes.data, on_dev),
              "solver_create_pseudo_sp")
        self.h = h

    def peek_v(self):
        out = np.empty((self.N, self.ncol), dtype=np.complex128 if self.cplx else np.float64, order="F")
        check(lib.chase_hip_solver_peek_v(self.h, self.ctx.h, out.ctypes.data, self.N), "peek_v")
        return out
