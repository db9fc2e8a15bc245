// gemm_sp_epilogue.h - the epilogue of the two single-precision GEMMs (gemm_sp_frame.h), included INSIDE the kernel body, after the
// K loop.  Expects in scope: the template parameters CPLX, WN, WIDE, E = CPLX ? 2 : 1, the kernel's Args a, its Place at and the
// accumulators f32x16 acc[2][WN][E].
//
// C = alpha acc + beta C in T = float (C fp32) or double (WIDE: the fp64 C and scalars of Args).  C/D map of the 32 x 32 tile:
// column = lane & 31, rows 8 g + 4 (lane >> 5) + (0..3) in registers 4 g .. 4 g + 3: a lane's four rows of a column are contiguous
// in C - 16-byte accesses where vecC allows and all four rows exist, guarded element accesses otherwise.  beta == 0: C is not read.
//
// Why text and not a function: as a function, force-inlined or left to the inliner, the accumulators reach it by reference and
// the compiler comes out with other code for the whole kernel (in some instantiations another K-loop schedule: complex fp32,
// 128 columns, op N 166 instead of 161 instructions per step, and the one-round panel product of a grid rank 1 % slower).  As
// text, every kernel's machine code is what it was with the epilogue written out in the kernel.  The static_asserts below pin
// the names this text takes from the kernel.
{
    static_assert(std::is_same<decltype(CPLX), bool>::value && std::is_same<decltype(WIDE), bool>::value &&
                  std::is_same<decltype(WN), int>::value && E == (CPLX ? 2 : 1), "gemm_sp_epilogue.h: template parameters");
    static_assert(std::is_same<decltype(a), const Args>::value && std::is_same<decltype(at), const Place>::value &&
                  std::is_same<decltype(acc), f32x16[2][WN][E]>::value, "gemm_sp_epilogue.h: a, at, acc of the kernel");
    using T = typename std::conditional<WIDE, double, float>::type;
    T* C; T ar, ai, br, bi;                    // (ar, ai) = alpha, (br, bi) = beta
    if constexpr (WIDE) { C = a.Cw; ar = a.war; ai = a.wai; br = a.wbr; bi = a.wbi; }
    else { C = a.C; ar = a.ar; ai = a.ai; br = a.br; bi = a.bi; }

    constexpr int V = 16 / sizeof(T);          // scalars per 16-byte vector
    const bool useC = (br != T(0)) || (bi != T(0));
    #pragma unroll
    for (int i = 0; i < 2; ++i)
        #pragma unroll
        for (int j = 0; j < WN; ++j) {
            const long col = at.n0 + at.wn * (32 * WN) + 32 * j + at.lr;
            if (col >= a.n) continue;
            #pragma unroll
            for (int g = 0; g < 4; ++g) {
                const long row = at.m0 + at.wm * 64 + 32 * i + 8 * g + 4 * at.lh;
                if (row >= a.m) continue;
                T* c = C + E * (row + col * a.ldc);
                const bool vec16 = a.vecC && row + 4 <= a.m;
                T o[4 * E], c0[4 * E];
                #pragma unroll
                for (int q = 0; q < 4 * E; ++q) c0[q] = T(0);
                if (useC) {
                    if (vec16) {
                        #pragma unroll
                        for (int q = 0; q < 4 * E / V; ++q) get16(c + V * q, c0 + V * q);
                    } else {
                        #pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (row + e < a.m) {
                                #pragma unroll
                                for (int s = 0; s < E; ++s) c0[E * e + s] = c[E * e + s];
                            }
                    }
                }
                #pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (CPLX) {
                        const T xr = (T)acc[i][j][0][4 * g + e], xi = (T)acc[i][j][1][4 * g + e];
                        T yr = ar * xr - ai * xi, yi = ar * xi + ai * xr;
                        if (useC) {
                            yr += br * c0[2 * e] - bi * c0[2 * e + 1];
                            yi += br * c0[2 * e + 1] + bi * c0[2 * e];
                        }
                        o[2 * e] = yr; o[2 * e + 1] = yi;
                    } else {
                        T y = ar * (T)acc[i][j][0][4 * g + e];
                        if (useC) y += br * c0[e];
                        o[e] = y;
                    }
                }
                if (vec16) {
                    #pragma unroll
                    for (int q = 0; q < 4 * E / V; ++q) put16(c + V * q, o + V * q);
                } else {
                    #pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (row + e < a.m) {
                            #pragma unroll
                            for (int s = 0; s < E; ++s) c[E * e + s] = o[E * e + s];
                        }
                }
            }
        }
}
