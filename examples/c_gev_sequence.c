/* c_gev_sequence.c — a plain C caller that solves a SEQUENCE of generalized problems H_k x = lambda S_k x, each pencil a small
 * perturbation of the one before (the k-point / SCF loop of a DFT code with a non-orthogonal basis), with ChASE's C interface
 * (include/chase_c_interface.h) on an MI355X.  The first pencil starts cold (mode 'R'); every later one starts from the previous
 * step's eigenvectors (mode 'A'):
 *
 *     dchase_gev_reduce_itype_         S_k = U^T U,  H_k <- U^{-T} H_k U^{-1}     (itype 1, factor 1; in place, host pointers)
 *     dchase_gev_starttransform_       V <- U V: the previous step's x, all nev + nex columns, become the start block   (k > 0)
 *     dchase_                          mode 'A' with the previous ritzv (k > 0), mode 'R' for k = 0
 *     dchase_gev_backtransform_itype_  V <- U^{-1} V, all nev + nex columns: the next step starts from them
 *
 * Per step the program prints the number of vectors the filter processed and the largest || H x - lambda S x ||_2 over the nev
 * pairs, recomputed on the host from the original matrices.
 *
 * usage:  c_gev_sequence [N [in.bin [out.bin]]]
 *   in.bin : H_0, S_0, H_1, S_1, H_2, S_2, N x N doubles each, column-major (default: a random symmetric H_0, a diagonally
 *            dominant S_0, and relative perturbations of 1e-3 from step to step)
 *   out.bin: per step lambda (nev), Y (N x nev, the reduced problem's vectors), X (N x nev), the reduced H_k and S_k-with-U (N x N each)
 * build:  gcc -O2 -std=c11 -Iinclude examples/c_gev_sequence.c -Lchase_amd/lib -lchase_hip -Wl,-rpath,$PWD/chase_amd/lib -lm
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "chase_c_interface.h"
#include "chase_hip_solver.h"

#define STEPS 3

static unsigned long long lcg_state = 88172645463325252ull;
static double lcg_uniform(void)            /* (0, 1) */
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return ((double)(lcg_state >> 11) + 0.5) / 9007199254740992.0;
}

int main(int argc, char** argv)
{
    int N = argc > 1 ? atoi(argv[1]) : 300, nev = 20, nex = 12, nevex = nev + nex;
    int deg = 20, init = 0, flag = 1, info = -1, itype = 1, factor = 1;
    double tol = 1e-10;
    char mode = 'R', opt = 'S', qr = 'C';
    if (N < nevex) return 2;
    const size_t nn = (size_t)N * N, nv = (size_t)N * nev;
    double *H = malloc(nn * sizeof *H), *S = malloc(nn * sizeof *S);
    double *Hk[STEPS], *Sk[STEPS];
    double* V = calloc((size_t)N * nevex, sizeof *V);
    double* Y = malloc(nv * sizeof *Y);
    double* lambda = calloc((size_t)nevex, sizeof *lambda);
    if (!H || !S || !V || !Y || !lambda) return 2;
    for (int p = 0; p < STEPS; ++p) {
        Hk[p] = malloc(nn * sizeof(double));
        Sk[p] = malloc(nn * sizeof(double));
        if (!Hk[p] || !Sk[p]) return 2;
    }

    if (argc > 2) {
        FILE* f = fopen(argv[2], "rb");
        int ok = f != NULL;
        for (int p = 0; ok && p < STEPS; ++p) ok = fread(Hk[p], sizeof(double), nn, f) == nn && fread(Sk[p], sizeof(double), nn, f) == nn;
        if (!ok) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        fclose(f);
    } else {
        for (int j = 0; j < N; ++j)
            for (int i = 0; i <= j; ++i) {
                const double h = lcg_uniform() - 0.5, s = (lcg_uniform() - 0.5) / N;
                Hk[0][i + (size_t)N * j] = Hk[0][j + (size_t)N * i] = (i == j) ? 10.0 * h + j : h;
                Sk[0][i + (size_t)N * j] = Sk[0][j + (size_t)N * i] = (i == j) ? 1.0 + 0.5 * lcg_uniform() : s;
            }
        for (int p = 1; p < STEPS; ++p)
            for (int j = 0; j < N; ++j)
                for (int i = 0; i <= j; ++i) {
                    const double dh = 1e-3 * (lcg_uniform() - 0.5), ds = 1e-3 * (lcg_uniform() - 0.5) / N;
                    Hk[p][i + (size_t)N * j] = Hk[p][j + (size_t)N * i] = Hk[p - 1][i + (size_t)N * j] + dh;
                    Sk[p][i + (size_t)N * j] = Sk[p][j + (size_t)N * i] = Sk[p - 1][i + (size_t)N * j] + ds;
                }
    }

    FILE* fout = argc > 3 ? fopen(argv[3], "wb") : NULL;
    if (argc > 3 && !fout) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }

    /* the solver keeps the pointers H, V and lambda: every step reduces its pencil INTO H and leaves its vectors in V */
    dchase_init_(&N, &nev, &nex, H, &N, V, lambda, &init);
    if (!init) { fprintf(stderr, "dchase_init_ failed\n"); return 3; }

    double filtered[STEPS], worst_all = 0.0, scale = 1.0;
    for (int p = 0; p < STEPS; ++p) {
        memcpy(H, Hk[p], nn * sizeof *H);
        memcpy(S, Sk[p], nn * sizeof *S);
        dchase_gev_reduce_itype_(&itype, &factor, &N, H, &N, S, &N, &info);
        if (info != 0) { fprintf(stderr, "dchase_gev_reduce_itype_: info = %d\n", info); return 3; }
        if (p > 0) {                       /* V holds the previous step's x, all nev + nex columns */
            dchase_gev_starttransform_(&itype, &N, &nevex, S, &N, V, &N, &info);
            if (info != 0) { fprintf(stderr, "dchase_gev_starttransform_: info = %d\n", info); return 3; }
            mode = 'A';
        }
        dchase_(&deg, &tol, &mode, &opt, &qr);
        filtered[p] = -1.0;
        chase_hip_solver_get(chase_hip_cshim_seq_solver(0), "filtered_vecs", &filtered[p]);
        memcpy(Y, V, nv * sizeof *Y);
        dchase_gev_backtransform_itype_(&itype, &N, &nevex, S, &N, V, &N, &info);
        if (info != 0) { fprintf(stderr, "dchase_gev_backtransform_itype_: info = %d\n", info); return 3; }

        double worst = 0.0;
        for (int j = 0; j < nev; ++j) {
            if (fabs(lambda[j]) > scale) scale = fabs(lambda[j]);
            double r2 = 0.0;
            for (int i = 0; i < N; ++i) {
                double s = 0.0;
                for (int k = 0; k < N; ++k) s += (Hk[p][i + (size_t)N * k] - lambda[j] * Sk[p][i + (size_t)N * k]) * V[k + (size_t)N * j];
                r2 += s * s;
            }
            printf("step %d pair %d: lambda = %.17g, || H x - lambda S x || = %.3e\n", p, j, lambda[j], sqrt(r2));
            if (sqrt(r2) > worst) worst = sqrt(r2);
        }
        printf("step %d (mode %c): %.0f filtered vectors, largest generalized residual %.3e\n", p, mode, filtered[p], worst);
        if (worst > worst_all) worst_all = worst;
        if (fout && (fwrite(lambda, sizeof *lambda, (size_t)nev, fout) != (size_t)nev || fwrite(Y, sizeof *Y, nv, fout) != nv ||
                     fwrite(V, sizeof *V, nv, fout) != nv || fwrite(H, sizeof *H, nn, fout) != nn || fwrite(S, sizeof *S, nn, fout) != nn)) {
            fprintf(stderr, "cannot write %s\n", argv[3]);
            return 2;
        }
    }
    dchase_finalize_(&flag);
    if (fout) fclose(fout);

    int warm_is_cheaper = 1;
    for (int p = 1; p < STEPS; ++p) warm_is_cheaper = warm_is_cheaper && filtered[p] > 0 && filtered[p] < filtered[0];
    for (int p = 0; p < STEPS; ++p) { free(Hk[p]); free(Sk[p]); }
    free(H); free(S); free(V); free(Y); free(lambda);
    if (!(worst_all < 1e-7 * scale) || flag || !warm_is_cheaper) { printf("FAILED\n"); return 1; }
    printf("C_GEV_SEQUENCE_OK\n");
    return 0;
}
