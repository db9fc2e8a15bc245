/* c_gev_sp.c — c_gev.c in single precision: a plain C caller that solves two generalized Hermitian-definite problems
 * H_k x = lambda S x with a complex fp32 pencil through ChASE's C interface (include/chase_c_interface.h) on an MI355X.  Nothing is
 * widened to fp64: the reduction, the solver (cchase_) and the back-transformation all work on float _Complex data.
 *
 *     cchase_gev_reduce_           S = U^H U,  H_0 <- U^{-H} H_0 U^{-1}      (in place, host pointers)
 *     cchase_                      mode 'R': the lowest nev pairs (lambda, y) of the reduced H_0
 *     cchase_gev_backtransform_    x = U^{-1} y
 * then a second pencil with the same S, 1e-3 away:
 *     cchase_gev_reduce_itype_     itype 1, factor 0: S still holds U, no second Cholesky;  H_1 <- U^{-H} H_1 U^{-1}
 *     cchase_                      mode 'A': starts from the first solve's y (S did not change, so they need no transform)
 *     cchase_gev_backtransform_
 * After each solve the largest || H_k x - lambda S x ||_2 over the nev pairs is recomputed on the host in double from copies of the
 * original fp32 matrices.
 *
 * usage:  c_gev_sp [N]
 * build:  gcc -O2 -std=c11 -Iinclude examples/c_gev_sp.c -Lchase_amd/lib -lchase_hip -Wl,-rpath,$PWD/chase_amd/lib -lm
 */
#include <complex.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "chase_c_interface.h"

typedef float _Complex cf;

static unsigned long long lcg_state = 88172645463325252ull;
static double lcg_uniform(void)            /* (0, 1) */
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}

/* max_j || H x_j - lambda_j S x_j ||_2 in double */
static double worst_residual(int N, int nev, const cf* H, const cf* S, const float* lambda, const cf* X)
{
    double worst = 0.0;
    for (int j = 0; j < nev; ++j) {
        double r2 = 0.0;
        for (int i = 0; i < N; ++i) {
            double _Complex s = 0.0;
            for (int k = 0; k < N; ++k)
                s += ((double _Complex)H[i + (size_t)N * k] - (double)lambda[j] * (double _Complex)S[i + (size_t)N * k]) *
                     (double _Complex)X[k + (size_t)N * j];
            r2 += creal(s) * creal(s) + cimag(s) * cimag(s);
        }
        if (sqrt(r2) > worst) worst = sqrt(r2);
    }
    return worst;
}

int main(int argc, char** argv)
{
    int N = argc > 1 ? atoi(argv[1]) : 300, nev = 20, nex = 12;
    int deg = 10, init = 0, flag = 1, info = -1, itype = 1, factor = 0;
    float tol = 1e-5f;
    char mode = 'R', opt = 'S', qr = 'C';
    if (N < nev + nex) return 2;
    const size_t nn = (size_t)N * N, nv = (size_t)N * (nev + nex);
    cf *H = malloc(nn * sizeof *H), *S = malloc(nn * sizeof *S), *H0 = malloc(nn * sizeof *H0), *H1 = malloc(nn * sizeof *H1),
       *S0 = malloc(nn * sizeof *S0);
    cf *V = calloc(nv, sizeof *V), *Y = malloc(nv * sizeof *Y);
    float* lambda = calloc((size_t)(nev + nex), sizeof *lambda);
    if (!H || !S || !H0 || !H1 || !S0 || !V || !Y || !lambda) return 2;

    /* || H || ~ 1: eigenvalues spread over (0, 1], a perturbation of 1 / N off the diagonal; S close to the identity */
    for (int j = 0; j < N; ++j)
        for (int i = 0; i <= j; ++i) {
            const float hr = (float)((lcg_uniform() - 0.5) / N), hi = (float)((lcg_uniform() - 0.5) / N);
            const float sr = (float)((lcg_uniform() - 0.5) / N), si = (float)((lcg_uniform() - 0.5) / N);
            const float dr = (float)((lcg_uniform() - 0.5) * 1e-3 / N), di = (float)((lcg_uniform() - 0.5) * 1e-3 / N);
            if (i == j) {
                H0[i + (size_t)N * j] = (float)(j + 1) / N + hr;
                H1[i + (size_t)N * j] = H0[i + (size_t)N * j] + dr;
                S0[i + (size_t)N * j] = 1.0f + 0.5f * (float)lcg_uniform();
            } else {
                H0[i + (size_t)N * j] = hr + hi * I;   H0[j + (size_t)N * i] = hr - hi * I;
                H1[i + (size_t)N * j] = H0[i + (size_t)N * j] + (dr + di * I);
                H1[j + (size_t)N * i] = conjf(H1[i + (size_t)N * j]);
                S0[i + (size_t)N * j] = sr + si * I;   S0[j + (size_t)N * i] = sr - si * I;
            }
        }
    memcpy(H, H0, nn * sizeof *H);
    memcpy(S, S0, nn * sizeof *S);

    cchase_init_(&N, &nev, &nex, H, &N, V, lambda, &init);
    if (!init) { fprintf(stderr, "cchase_init_ failed\n"); return 3; }

    /* ---- the first pencil, cold ---- */
    cchase_gev_reduce_(&N, H, &N, S, &N, &info);
    if (info != 0) { fprintf(stderr, "cchase_gev_reduce_: info = %d\n", info); return 3; }
    cchase_(&deg, &tol, &mode, &opt, &qr);
    memcpy(Y, V, nv * sizeof *Y);                      /* all nev + nex columns: the start block of the next solve */
    cchase_gev_backtransform_(&N, &nev, S, &N, V, &N, &info);
    if (info != 0) { fprintf(stderr, "cchase_gev_backtransform_: info = %d\n", info); return 3; }
    const double w0 = worst_residual(N, nev, H0, S0, lambda, V);
    printf("pencil 0 (mode R): lambda_0 = %.7g, largest generalized residual %.3e\n", lambda[0], w0);

    /* ---- the second pencil: S unchanged, factor = 0, warm start ---- */
    memcpy(H, H1, nn * sizeof *H);
    cchase_gev_reduce_itype_(&itype, &factor, &N, H, &N, S, &N, &info);
    if (info != 0) { fprintf(stderr, "cchase_gev_reduce_itype_: info = %d\n", info); return 3; }
    memcpy(V, Y, nv * sizeof *V);
    mode = 'A';
    cchase_(&deg, &tol, &mode, &opt, &qr);
    cchase_gev_backtransform_(&N, &nev, S, &N, V, &N, &info);
    if (info != 0) { fprintf(stderr, "cchase_gev_backtransform_: info = %d\n", info); return 3; }
    const double w1 = worst_residual(N, nev, H1, S0, lambda, V);
    printf("pencil 1 (mode A): lambda_0 = %.7g, largest generalized residual %.3e\n", lambda[0], w1);
    cchase_finalize_(&flag);

    /* itype 2 is not served in single precision */
    itype = 2;
    cchase_gev_reduce_itype_(&itype, &factor, &N, H, &N, S, &N, &info);
    const int refused = info < 0;

    const double worst = w0 > w1 ? w0 : w1;
    printf("largest generalized residual %.3e\n", worst);
    free(H); free(S); free(H0); free(H1); free(S0); free(V); free(Y); free(lambda);
    /* || C || ~ 1 and tol = 1e-5: the solver stops at reduced residuals below 1e-5, the fp32 reduction adds a few 1e-6 */
    if (!(worst < 1e-4) || flag || !refused) { printf("FAILED\n"); return 1; }
    printf("OK\n");
    return 0;
}
