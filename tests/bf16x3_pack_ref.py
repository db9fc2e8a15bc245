"""numpy restatement of the packed bf16x3 operand (include/chase_hip.h, chase_amd/csrc/gemm_mfma_bf16x3p.hip), on the split of
tests/bf16x3_ref.py.

An m x k matrix, rows padded to P = ceil(m / 128) panels, k to T = ceil(k / 16) steps.  Block (panel p, step t) is at 16-byte piece
(p T + t) * planes * 256, planes = 3 (real: parts 1, 2, 3) or 6 (complex: re 1, 2, 3, im 1, 2, 3), 256 pieces per plane.  Piece
(row, h) of a plane sits at 2 row + (h ^ bit 2 of row ^ bit 3 of row) and holds the part's eight bf16 numbers of matrix row
128 p + row at k = 16 t + 8 h + 0..7.  Padding is zero."""
import numpy as np

import bf16x3_ref as R

BM, BK = 128, 16


def planes(cplx):
    return 6 if cplx else 3


def dims(m, k):
    return (m + BM - 1) // BM, (k + BK - 1) // BK


def pack_bytes(m, k, cplx):
    if m == 0 or k == 0:
        return 0
    P, T = dims(m, k)
    return P * T * planes(cplx) * 256 * 16


def piece(row, h):
    return 2 * row + (h ^ ((row >> 2) & 1) ^ ((row >> 3) & 1))


def _bf16_bits(x):
    """fp32 array of bf16 numbers -> their 16 bits"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert np.all((u & 0xFFFF) == 0)
    return (u >> 16).astype(np.uint16)


def _index(m, k, cplx):
    """uint16 index into the buffer of (plane s, row i, column j), as an array [planes, P 128, T 16]"""
    P, T = dims(m, k)
    i = np.arange(P * BM)[:, None]
    j = np.arange(T * BK)[None, :]
    p, row, t, h, e = i // BM, i % BM, j // BK, (j % BK) // 8, j % 8
    base = (p * T + t) * (planes(cplx) * 256) + piece(row, h)                # in pieces
    s = np.arange(planes(cplx))[:, None, None]
    return ((base[None] + 256 * s) * 8 + e[None]).astype(np.int64)


def part_planes(A):
    """the planes of a real or complex fp32 matrix, as fp32 arrays [planes, m, k]"""
    A = np.asarray(A)
    if np.iscomplexobj(A):
        A = A.astype(np.complex64)
        return np.stack(R.split3(np.ascontiguousarray(A.real)) + R.split3(np.ascontiguousarray(A.imag)))
    return np.stack(R.split3(A.astype(np.float32)))


def pack(A):
    """the packed image of the fp32 / complex fp32 matrix A (m x k), as a uint8 array of pack_bytes(m, k) bytes"""
    A = np.asarray(A)
    m, k = A.shape
    cplx = np.iscomplexobj(A)
    out = np.zeros(pack_bytes(m, k, cplx) // 2, np.uint16)
    if out.size == 0:
        return out.view(np.uint8)
    idx = _index(m, k, cplx)
    out[idx[:, :m, :k].ravel()] = _bf16_bits(part_planes(A)).ravel()
    return out.view(np.uint8)


def unpack(buf, m, k, cplx):
    """the inverse: the planes [planes, m, k] as fp32 and the uint16 words of the padding (all of them must be zero)"""
    w = np.frombuffer(np.ascontiguousarray(buf), np.uint16)
    assert w.size * 2 == pack_bytes(m, k, cplx)
    idx = _index(m, k, cplx)
    parts = (w[idx[:, :m, :k]].astype(np.uint32) << 16).view(np.float32)
    seen = np.zeros(w.size, bool)
    seen[idx[:, :m, :k].ravel()] = True
    return parts, w[~seen]
