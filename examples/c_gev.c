/* c_gev.c — a plain C caller that solves a generalized Hermitian-definite problem H x = lambda S x with ChASE's C interface
 * (include/chase_c_interface.h) on an MI355X.  The reference does this with three ScaLAPACK calls around the solver
 * (docs/example/gev.rst: ppotrf, phegst, ptrtrs); here they are dchase_gev_reduce_ and dchase_gev_backtransform_:
 *
 *     dchase_gev_reduce_          S = U^T U,  H <- U^{-T} H U^{-1}        (in place, host pointers)
 *     dchase_init_ / dchase_ / dchase_finalize_   on the reduced H: the lowest nev pairs (lambda, y)
 *     dchase_gev_backtransform_   x = U^{-1} y                            (the vectors come out S-orthonormal)
 *
 * and the largest || H x - lambda S x ||_2 over the nev pairs is recomputed on the host from copies of the original matrices.
 *
 * usage:  c_gev [N [in.bin [out.bin]]]
 *   in.bin : H then S, N x N doubles each, column-major (default: a random symmetric H and a diagonally dominant S)
 *   out.bin: lambda (nev), Y (N x nev, the reduced problem's vectors), X (N x nev), then the reduced H and S-with-U (N x N each)
 * build:  gcc -O2 -std=c11 -Iinclude examples/c_gev.c -Lchase_amd/lib -lchase_hip -Wl,-rpath,$PWD/chase_amd/lib -lm
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "chase_c_interface.h"

static unsigned long long lcg_state = 88172645463325252ull;
static double lcg_uniform(void)            /* (0, 1) */
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}

int main(int argc, char** argv)
{
    int N = argc > 1 ? atoi(argv[1]) : 300, nev = 20, nex = 12;
    int deg = 20, init = 0, flag = 1, info = -1;
    double tol = 1e-10;
    char mode = 'R', opt = 'S', qr = 'C';
    if (N < nev + nex) return 2;
    const size_t nn = (size_t)N * N, nv = (size_t)N * nev;
    double *H = malloc(nn * sizeof *H), *S = malloc(nn * sizeof *S), *H0 = malloc(nn * sizeof *H0), *S0 = malloc(nn * sizeof *S0);
    double* V = calloc((size_t)N * (nev + nex), sizeof *V);
    double* Y = malloc(nv * sizeof *Y);
    double* lambda = calloc((size_t)(nev + nex), sizeof *lambda);
    if (!H || !S || !H0 || !S0 || !V || !Y || !lambda) return 2;

    if (argc > 2) {
        FILE* f = fopen(argv[2], "rb");
        if (!f || fread(H, sizeof *H, nn, f) != nn || fread(S, sizeof *S, nn, f) != nn) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        fclose(f);
    } else {
        for (int j = 0; j < N; ++j)
            for (int i = 0; i <= j; ++i) {
                const double h = lcg_uniform() - 0.5, s = (lcg_uniform() - 0.5) / N;
                H[i + (size_t)N * j] = H[j + (size_t)N * i] = (i == j) ? 10.0 * h + j : h;
                S[i + (size_t)N * j] = S[j + (size_t)N * i] = (i == j) ? 1.0 + 0.5 * lcg_uniform() : s;
            }
    }
    memcpy(H0, H, nn * sizeof *H);
    memcpy(S0, S, nn * sizeof *S);

    dchase_gev_reduce_(&N, H, &N, S, &N, &info);
    if (info != 0) { fprintf(stderr, "dchase_gev_reduce_: info = %d\n", info); return 3; }

    dchase_init_(&N, &nev, &nex, H, &N, V, lambda, &init);
    if (!init) { fprintf(stderr, "dchase_init_ failed\n"); return 3; }
    dchase_(&deg, &tol, &mode, &opt, &qr);
    dchase_finalize_(&flag);
    memcpy(Y, V, nv * sizeof *Y);

    dchase_gev_backtransform_(&N, &nev, S, &N, V, &N, &info);
    if (info != 0) { fprintf(stderr, "dchase_gev_backtransform_: info = %d\n", info); return 3; }

    double worst = 0.0, scale = 1.0;
    for (int j = 0; j < nev; ++j) {
        if (fabs(lambda[j]) > scale) scale = fabs(lambda[j]);
        double r2 = 0.0;
        for (int i = 0; i < N; ++i) {
            double s = 0.0;
            for (int k = 0; k < N; ++k) s += (H0[i + (size_t)N * k] - lambda[j] * S0[i + (size_t)N * k]) * V[k + (size_t)N * j];
            r2 += s * s;
        }
        printf("pair %d: lambda = %.17g, || H x - lambda S x || = %.3e\n", j, lambda[j], sqrt(r2));
        if (sqrt(r2) > worst) worst = sqrt(r2);
    }
    printf("largest generalized residual %.3e\n", worst);

    if (argc > 3) {
        FILE* f = fopen(argv[3], "wb");
        if (!f || fwrite(lambda, sizeof *lambda, (size_t)nev, f) != (size_t)nev || fwrite(Y, sizeof *Y, nv, f) != nv ||
            fwrite(V, sizeof *V, nv, f) != nv || fwrite(H, sizeof *H, nn, f) != nn || fwrite(S, sizeof *S, nn, f) != nn) {
            fprintf(stderr, "cannot write %s\n", argv[3]);
            return 2;
        }
        fclose(f);
    }

    /* an indefinite S is reported, not factorised: pivot 3 */
    memcpy(S, S0, nn * sizeof *S);
    memcpy(H, H0, nn * sizeof *H);
    S[2 + (size_t)N * 2] = -1.0;
    dchase_gev_reduce_(&N, H, &N, S, &N, &info);
    printf("indefinite S: info = %d\n", info);
    const int untouched = memcmp(H, H0, nn * sizeof *H) == 0;

    free(H); free(S); free(H0); free(S0); free(V); free(Y); free(lambda);
    if (!(worst < 1e-7 * scale) || flag || info != 3 || !untouched) { printf("FAILED\n"); return 1; }
    printf("C_GEV_OK\n");
    return 0;
}
