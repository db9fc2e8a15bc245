"""Reference side of the row-distributed Householder QR (chase_hip_houseqr_dist, chase_amd/csrc/hhqr.hip): numpy / scipy only,
no GPU, no chase_amd.  Imported by tests/dist_qr_scenarios.py, tests/test_gpu_dist_qr.py and - the model and the shapes are
checked themselves - tests/test_dist_qr_refs_cpu.py.  The checkers (qr_ratios, qr_vs_lapack_ratios, same_padding, same_bits) and
the inputs (qr_cases) are those of tests/dense_chain_refs.py: the distributed QR is held to what its single-GPU twin is held to.

The rows of an m x n block are dealt to the ranks of a column group in STACKED order: rank 0's rows first, then rank 1's, ...;
rank r holds counts[r] rows (0 is allowed anywhere) starting at stacked row offsets[r].  The pivot of column j is stacked row j."""
import numpy as np
import dense_chain_refs as D

HMAX = 48                                   # capacity of the panel kernels: CHASE_HOUSEHOLDER_NB is clamped to it
PAD = 3                                     # rows of canary under every rank's block: ldv = mloc + PAD

# (name, nprow, npcol, rows per rank of the column group, n).  What each is for:
#   five_passes     the 256-stride loops take five passes, two panels (32, 8), no communication
#   two_ranks       two passes, three panels (32, 32, 6), every pivot on rank 0
#   replicas        two grid columns factor the same block redundantly: their Q must be equal bit for bit
#   empty_and_one   a rank without rows inside the order, a rank with one row
#   square          m == n: every rank shorter than a panel, pivots cross three rank boundaries, nothing under the last pivot
#   tiny, tiny_empty_last   the smallest shapes: one short panel; the block rule's trailing empty rank
CASES = [("five_passes", 1, 1, (1100,), 40),
         ("two_ranks", 2, 1, (300, 300), 70),
         ("replicas", 2, 2, (257, 343), 70),
         ("empty_and_one", 4, 1, (300, 0, 299, 1), 70),
         ("square", 4, 2, (20, 40, 10, 60), 130),
         ("tiny", 3, 1, (3, 3, 3), 4),
         ("tiny_empty_last", 4, 1, (3, 3, 3, 0), 4)]
CASE = {c[0]: c for c in CASES}
PANEL_WIDTHS = [2, 17, 48, 200]             # CHASE_HOUSEHOLDER_NB on the two_ranks case; 200 is clamped to 48
SHAPES = sorted({(sum(c[3]), c[4]) for c in CASES})          # (m, n) of the stacked blocks: (9, 4) (130, 130) (600, 70) (1100, 40)


def panel_width(nb):
    """householder_nb() of hhqr.hip for CHASE_HOUSEHOLDER_NB = nb (None: unset)"""
    if nb is None or nb <= 0:
        return 32
    return max(2, min(int(nb), HMAX))


def stacked_split(m, counts):
    """-> (offsets, slices): rank r holds the stacked rows slices[r] = offsets[r] : offsets[r] + counts[r]"""
    counts = [int(c) for c in counts]
    assert all(c >= 0 for c in counts) and sum(counts) == m, (m, counts)
    offsets = [int(o) for o in np.concatenate([[0], np.cumsum(counts)[:-1]])]
    return offsets, [slice(o, o + c) for o, c in zip(offsets, counts)]


def inputs(name, cplx):
    """the QR inputs of one case, in stacked order: kind -> m x n (the kinds of dense_chain_refs.qr_cases, seeded per shape)"""
    _, _, _, counts, n = CASE[name]
    m = sum(counts)
    return D.qr_cases(np.random.default_rng(D.seed_of(3, m, n, cplx)), m, n, cplx)


def _larft(G, tau):
    """LAPACK xLARFT (forward, columnwise) from G = V^H V, as larft_kernel has it"""
    nb = len(tau)
    T = np.zeros((nb, nb), dtype=G.dtype)
    for i in range(nb):
        T[:i, i] = -tau[i] * (T[:i, :i] @ G[:i, i])
        T[i, i] = tau[i]
    return T


def model_houseqr_dist(V, counts, nb=None, pad=PAD, drop_rows_from=None, wrong_ld=False):
    """chase_hip_houseqr_dist in plain numpy, rank by rank on buffers of ldv = mloc + pad rows whose pad rows hold the canary:
    per column ONE fused sum over the ranks (|x|^2 below the pivot, alpha, x^H A_panel below the pivot, the pivot row), every rank
    deriving beta / tau / scale from it; per panel G = V^H V -> T (larft) and W = V^H C in one sum, C -= V T^H W, the panel's
    reflectors stored over the factored columns; Q by backward accumulation with one sum per panel.
    -> the list of the ranks' buffers (ldv x n; rows < mloc are Q's rows).
    Seeded defects: drop_rows_from = k leaves each rank's rows from k on out of the column sums (a strided loop that never takes
    its second pass); wrong_ld stores the panel's reflectors with the extent mloc where the leading dimension ldv belongs."""
    V = np.asarray(V)
    m, n = V.shape
    dt = V.dtype
    offsets, slices = stacked_split(m, counts)
    P = len(counts)
    PNB = panel_width(nb)
    A = [D.padded(V[s], c + pad) for s, c in zip(slices, counts)]
    tau = np.zeros(n, dtype=dt)
    Ts = []
    for j0 in range(0, n, PNB):
        w = min(PNB, n - j0)
        pend = j0 + w
        Vb = [np.zeros((c, w), dtype=dt) for c in counts]
        for j in range(j0, pend):
            nc = pend - j - 1
            lp = [j - o for o in offsets]                             # local pivot row (may lie outside [0, mloc))
            lo = [max(l + 1, 0) for l in lp]
            own = [0 <= l < c for l, c in zip(lp, counts)]
            xn2, alpha = 0.0, dt.type(0)
            dots, piv = np.zeros(nc, dtype=dt), np.zeros(nc, dtype=dt)
            for r in range(P):
                hi = counts[r] if drop_rows_from is None else min(counts[r], max(drop_rows_from, lo[r]))
                x = A[r][lo[r]:hi, j]
                xn2 += float(np.sum(x.real ** 2 + x.imag ** 2))
                dots += x.conj() @ A[r][lo[r]:hi, j + 1:pend]
                if own[r]:
                    alpha = A[r][lp[r], j]
                    piv += A[r][lp[r], j + 1:pend]
            ar, ai = float(np.real(alpha)), float(np.imag(alpha))
            ident = xn2 == 0.0 and ai == 0.0                           # H = I
            t = scale = dt.type(0)
            if not ident:
                nrm = np.sqrt(ar * ar + ai * ai + xn2)
                beta = -nrm if ar >= 0.0 else nrm
                t = dt.type(complex((beta - ar) / beta, -ai / beta) if V.dtype.kind == "c" else (beta - ar) / beta)
                scale = dt.type(1.0 / (alpha - beta))
            tau[j] = t
            f = np.conj(t) * (np.conj(scale) * dots + piv)             # conj(tau) v^H a_c
            for r in range(P):
                v = Vb[r][:, j - j0]
                v[lo[r]:] = A[r][lo[r]:counts[r], j] * scale
                if own[r]:
                    v[lp[r]] = 1.0
                if ident or nc == 0:
                    continue
                A[r][lo[r]:counts[r], j + 1:pend] -= np.outer(A[r][lo[r]:counts[r], j], f * scale)
                if own[r]:
                    A[r][lp[r], j + 1:pend] -= f
        G = sum(Vb[r].conj().T @ Vb[r] for r in range(P))
        T = _larft(G, tau[j0:pend])
        Ts.append(T)
        if pend < n:                                                   # C -= V T^H (V^H C)
            W = sum(Vb[r].conj().T @ A[r][:counts[r], pend:] for r in range(P))
            W2 = T.conj().T @ W
            for r in range(P):
                A[r][:counts[r], pend:] -= Vb[r] @ W2
        for r in range(P):                                             # copy2d(Vb, mloc -> A[:, j0:], ldv)
            ldv, c = A[r].shape[0], counts[r]
            flat = A[r].reshape(-1, order="F")
            assert np.shares_memory(flat, A[r])
            ld = c if wrong_ld else ldv
            for k in range(w):
                flat[j0 * ldv + k * ld: j0 * ldv + k * ld + c] = Vb[r][:, k]
    Q = [np.zeros((c, n), dtype=dt) for c in counts]
    for r in range(P):
        for i in range(counts[r]):
            if offsets[r] + i < n:
                Q[r][i, offsets[r] + i] = 1.0
    for p in reversed(range(len(Ts))):                                 # Q = H_0 ... H_{n-1} I(:, 0:n), backwards over the panels
        j0 = p * PNB
        w = Ts[p].shape[0]
        Vp = [A[r][:counts[r], j0:j0 + w] for r in range(P)]
        W = sum(Vp[r].conj().T @ Q[r][:, j0:] for r in range(P))
        W2 = Ts[p] @ W
        for r in range(P):
            Q[r][:, j0:] -= Vp[r] @ W2
    for r in range(P):
        A[r][:counts[r]] = Q[r]
    return A


def gather(bufs, counts):
    """the ranks' buffers -> Q in stacked order (the pad rows left out)"""
    return np.concatenate([np.asarray(b)[:c] for b, c in zip(bufs, counts)], axis=0)


def padding_intact(bufs, counts):
    return all(D.same_padding(b, c) for b, c in zip(bufs, counts))


def ratios(V, Q, kind):
    """qr_ratios for every input; for the well-conditioned "random" one of a tall block the comparison with LAPACK's Q of the
    stacked-order matrix as well (m == n is left out: kappa_2 of a square random matrix reaches 939 at n = 130, and qr_g_raw asks
    for <= 1e3 - too close to be a property of the shape)"""
    out = dict(D.qr_ratios(V, Q))
    if kind == "random" and V.shape[0] > V.shape[1] and "finite" not in out:
        out.update(D.qr_vs_lapack_ratios(V, Q))
    return out
