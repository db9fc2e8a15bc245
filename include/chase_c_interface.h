/* chase_c_interface.h — the application-facing C / Fortran-style entry points of ChASE for the sequential fp64 paths,
 * served by the MI355X backend.  Same names, argument order and meaning as the reference's
 * interface/chase_c_interface.h:13-41 (dchase_init_, dchase_, dchase_finalize_ and the z variants; all arguments by
 * pointer, Fortran convention), so an application linked against ChASE's C interface (FLEUR / YAMBO style callers,
 * examples/4_interface) relinks against libchase_hip.so unchanged.
 *   init     : N, nev, nex, H (N x N, ldh, host), V (N x (nev+nex), host, may hold approximate vectors), ritzv;
 *              *init = 1 on success, 0 on failure (chase_hip_last_error() has the text)
 *   solve    : deg, tol, mode ('R' random start / 'A' approximate vectors in V), opt ('S' optimise degrees / 'X' not),
 *              qr ('C' CholQR / 'H' Householder)            (interface/chase_c_interface.cpp:444-466)
 *   finalize : *flag = 1
 *   *_internal_      : the interface owns V and ritzv (interface/chase_c_interface.h:25-32); read the result with
 *   ?chase_get_eigenpairs_(LEigsV, ld, ritzv): first nev eigenvectors (N x nev, ld >= N) and Ritz values (:177-181)
 *   zchase_init_pseudo_[internal_] / zchase_pseudo_ : pseudo-Hermitian (Bethe-Salpeter) problems through chase::Solve_pseudo;
 *              V has 2*(nev+nex) columns, ritzv 2*(nev+nex) entries (:44-58); zchase_ solves whichever type was initialised
 * The GPU is chosen by CHASE_HIP_DEVICE (default 0).
 *   schase_* / cchase_* : the same sequence in single precision (interface/chase_c_interface.h:19-41,178-212): H, V and ritzv
 *              are float / float _Complex / float, tol is a float; served by the single-precision solver
 *              (chase_hip_solver_create_sp), whose Ritz values are converted at this boundary.
 *   cchase_init_pseudo_[internal_] / cchase_pseudo_ : single-precision pseudo-Hermitian problems (:46-57) on
 *              chase_hip_solver_create_pseudo_sp; V has 2*(nev+nex) columns, ritzv 2*(nev+nex) floats; the slot rules are those of z:
 *              cchase_ solves whichever type was initialised, cchase_get_eigenpairs_ / cchase_finalize_ serve whichever is live.
 *              The p[sc]chase grid names are not provided.
 *
 * Distributed entry points (interface/chase_c_interface.h:61-65,95-99,126-128,149,177-195): every p?chase_init* of the
 * reference takes an MPI_Comm* and builds the 2D grid from it.  libchase_hip.so exports the same entry points with the
 * communicator replaced by a chase_hip_grid* (suffix _hip_; the grid carries dims, coordinates and the RCCL row / column
 * communicators; tell the shim the grid's device context first: chase_hip_cshim_use_ctx), and libchase_hip_mpi.so (built
 * when mpi.h is found; chase_amd/host/c_interface_mpi.c) exports the reference's exact MPI_Comm* signatures on top of
 * them.  H is the caller's HOST block of the local rows / columns (m x n, ldh); V the host block of local rows
 * (m x (nev+nex), ld = m; 2*(nev+nex) columns for pseudo-Hermitian problems), read when mode == 'A' and written by the
 * solve; mbsize / nbsize select the block-cyclic layout, irsrc / icsrc must be 0.  After init the names are the
 * reference's: p?chase_, p?chase_get_eigenpairs_ (local rows of the first nev vectors), p?chase_finalize_,
 * p?chase_readHam_ / p?chase_wrtHam_ (the local shard from / to a raw column-major N x N file). */
#ifndef CHASE_C_INTERFACE_HIP_H
#define CHASE_C_INTERFACE_HIP_H
#ifdef __cplusplus
extern "C" {
#endif
void dchase_init_(int* N, int* nev, int* nex, double* H, int* ldh, double* V, double* ritzv, int* init);
void dchase_(int* deg, double* tol, char* mode, char* opt, char* qr);
void dchase_finalize_(int* flag);
void zchase_init_(int* N, int* nev, int* nex, void* H, int* ldh, void* V, double* ritzv, int* init);
void zchase_(int* deg, double* tol, char* mode, char* opt, char* qr);
void zchase_finalize_(int* flag);
void dchase_init_internal_(int* N, int* nev, int* nex, double* H, int* ldh, int* init);
void zchase_init_internal_(int* N, int* nev, int* nex, void* H, int* ldh, int* init);
void zchase_init_pseudo_(int* N, int* nev, int* nex, void* H, int* ldh, void* V, double* ritzv, int* init);
void zchase_init_pseudo_internal_(int* N, int* nev, int* nex, void* H, int* ldh, int* init);
void zchase_pseudo_(int* deg, double* tol, char* mode, char* opt, char* qr);
void dchase_get_eigenpairs_(double* LEigsV, int* ld, double* ritzv);
void zchase_get_eigenpairs_(void* LEigsV, int* ld, double* ritzv);
void schase_init_(int* N, int* nev, int* nex, float* H, int* ldh, float* V, float* ritzv, int* init);
void schase_init_internal_(int* N, int* nev, int* nex, float* H, int* ldh, int* init);
void schase_(int* deg, float* tol, char* mode, char* opt, char* qr);
void schase_finalize_(int* flag);
void schase_get_eigenpairs_(float* LEigsV, int* ld, float* ritzv);
void cchase_init_(int* N, int* nev, int* nex, void* H, int* ldh, void* V, float* ritzv, int* init);
void cchase_init_internal_(int* N, int* nev, int* nex, void* H, int* ldh, int* init);
void cchase_init_pseudo_(int* N, int* nev, int* nex, void* H, int* ldh, void* V, float* ritzv, int* init);
void cchase_init_pseudo_internal_(int* N, int* nev, int* nex, void* H, int* ldh, int* init);
void cchase_pseudo_(int* deg, float* tol, char* mode, char* opt, char* qr);
void cchase_(int* deg, float* tol, char* mode, char* opt, char* qr);
void cchase_finalize_(int* flag);
void cchase_get_eigenpairs_(void* LEigsV, int* ld, float* ritzv);
/* Generalized Hermitian-definite problems H x = lambda S x (fp64, one GPU): the three ScaLAPACK calls of the reference's
 * docs/example/gev.rst.  Host pointers, in place, every argument by pointer.  reduce: S (Hermitian positive definite, upper
 * triangle read) becomes its Cholesky factor U in the upper triangle (S = U^H U; the strictly lower triangle is left alone), H
 * (upper triangle read) becomes U^{-H} H U^{-1}, both triangles, exactly Hermitian.  backtransform: V (N x ncols) <- U^{-1} V.
 * *info: 0, the index of the first non-positive pivot of S (H and S are then unchanged), or a negative CHASE_HIP_* code.
 * Sequence: ?chase_gev_reduce_ -> ?chase_init_ / ?chase_ / ?chase_finalize_ on the reduced H -> ?chase_gev_backtransform_ on
 * the eigenvectors; the Ritz values are those of (H, S), the vectors come out S-orthonormal.
 * The _itype forms take LAPACK's problem type: 1, H x = lambda S x; 2, H S x = lambda x; 3, S H x = lambda x (2 and 3 reduce to
 * U H U^H).  factor = 1 factors S as reduce does; factor = 0 says S already holds U - the overlap matrix of a sequence did not
 * change - and only H is reduced.  backtransform_itype: V <- U^{-1} V (itype 1, 2) or U^H V (itype 3).  starttransform is its
 * inverse, V <- U V (itype 1, 2) or U^{-H} V (itype 3): it makes approximate eigenvectors of the pencil a start block of the
 * reduced problem.  A warm step of a sequence: reduce_itype on the new pencil -> starttransform of the previous step's
 * back-transformed block, all nev + nex columns, into V -> ?chase_ with mode 'A' and the previous ritzv -> backtransform_itype
 * (examples/c_gev_sequence.c).  itype outside 1 .. 3 or factor outside 0 / 1: *info = CHASE_HIP_EINVAL.
 * schase_gev_* / cchase_gev_*: the same entry points on float / float _Complex matrices, served by the single-precision drivers
 * (chase_hip_gev_reduce_sp and friends: nothing is widened to fp64) and used around schase_init_ / schase_ / schase_finalize_
 * (examples/c_gev_sp.c).  They cover itype 1 only: itype 2 or 3 gives *info = CHASE_HIP_EINVAL.
 * Not provided: grid solvers, pseudo-Hermitian pencils. */
void dchase_gev_reduce_(int* N, double* H, int* ldh, double* S, int* lds, int* info);
void zchase_gev_reduce_(int* N, void* H, int* ldh, void* S, int* lds, int* info);
void dchase_gev_backtransform_(int* N, int* ncols, double* U, int* ldu, double* V, int* ldv, int* info);
void zchase_gev_backtransform_(int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info);
void dchase_gev_reduce_itype_(int* itype, int* factor, int* N, double* H, int* ldh, double* S, int* lds, int* info);
void zchase_gev_reduce_itype_(int* itype, int* factor, int* N, void* H, int* ldh, void* S, int* lds, int* info);
void dchase_gev_backtransform_itype_(int* itype, int* N, int* ncols, double* U, int* ldu, double* V, int* ldv, int* info);
void zchase_gev_backtransform_itype_(int* itype, int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info);
void dchase_gev_starttransform_(int* itype, int* N, int* ncols, double* U, int* ldu, double* V, int* ldv, int* info);
void zchase_gev_starttransform_(int* itype, int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info);
void schase_gev_reduce_(int* N, float* H, int* ldh, float* S, int* lds, int* info);
void cchase_gev_reduce_(int* N, void* H, int* ldh, void* S, int* lds, int* info);
void schase_gev_backtransform_(int* N, int* ncols, float* U, int* ldu, float* V, int* ldv, int* info);
void cchase_gev_backtransform_(int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info);
void schase_gev_reduce_itype_(int* itype, int* factor, int* N, float* H, int* ldh, float* S, int* lds, int* info);
void cchase_gev_reduce_itype_(int* itype, int* factor, int* N, void* H, int* ldh, void* S, int* lds, int* info);
void schase_gev_backtransform_itype_(int* itype, int* N, int* ncols, float* U, int* ldu, float* V, int* ldv, int* info);
void cchase_gev_backtransform_itype_(int* itype, int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info);
void schase_gev_starttransform_(int* itype, int* N, int* ncols, float* U, int* ldu, float* V, int* ldv, int* info);
void cchase_gev_starttransform_(int* itype, int* N, int* ncols, void* U, int* ldu, void* V, int* ldv, int* info);
void chase_enable_sym_check_(int* flag);    /* interface/chase_c_interface.cpp:4055: flag kept for callers that set it */
/* unified configuration setters and build queries (interface/chase_c_interface.h:207-238): act on the live solver instance
 * (sequential or distributed), silent when none is initialised */
void chase_set_tol_(double* tol);
void chase_set_deg_(int* deg);
void chase_set_max_deg_(int* max_deg);
void chase_set_deg_extra_(int* deg_extra);
void chase_set_max_iter_(int* max_iter);
void chase_set_lanczos_iter_(int* lanczos_iter);
void chase_set_num_lanczos_(int* num_lanczos);
void chase_set_approx_(int* flag);
void chase_set_opt_(int* flag);
void chase_set_cholqr_(int* flag);
void chase_set_decaying_rate_(float* decaying_rate);
void chase_set_cluster_aware_degrees_(int* flag);
void chase_set_upperb_scale_rate_(float* upperb_scale_rate);
void chase_get_version_(char* version, int* len);
void chase_has_cuda_(int* flag);          /* 0 */
void chase_has_nccl_(int* flag);          /* 1: the NCCL API is served by RCCL */
void chase_has_scalapack_(int* flag);     /* 0 */
void chase_has_mpi_(int* flag);           /* 1 when libchase_hip_mpi.so is loaded in the process */
void chase_print_config_(void);
void dchase_readHam_(const char* filename);  /* aliases of p?chase_readHam_ */
void zchase_readHam_(const char* filename);
void schase_readHam_(const char* filename);  /* no single-precision grid solver to read into: says so on stderr */
void cchase_readHam_(const char* filename);

/* ---- distributed (one process per GPU) ---- */
struct chase_hip_grid;
struct chase_hip_ctx;
struct chase_hip_solver;
int chase_hip_cshim_use_ctx(struct chase_hip_ctx* ctx, int own); /* context of the NEXT _hip_ init; own: finalize destroys grid + ctx */
struct chase_hip_solver* chase_hip_cshim_dist_solver(int cplx); /* the live distributed solver (chase_hip_solver.h), or NULL */
/* 1: every thread that calls a p?chase_init*_hip_ entry point from now on is one RANK of a grid living in this process (one
 * thread per GPU) with a solver of its own; 0 (default): ONE solver per type in the process, replaced by the next init from
 * any thread - the reference's static members (interface/chase_c_interface.cpp:905-1290).  Returns the previous setting. */
int chase_hip_cshim_thread_ranks(int on);
struct chase_hip_solver* chase_hip_cshim_seq_solver(int kind); /* live sequential solver: 0 real, 1 complex, 2 complex pseudo-Hermitian, 3 / 4 single-precision real / complex, 5 single-precision complex pseudo-Hermitian */
void pdchase_init_hip_(int* N, int* nev, int* nex, int* m, int* n, double* H, int* ldh, double* V, double* ritzv,
                       struct chase_hip_grid* grid, int* init);
void pdchase_init_internal_hip_(int* N, int* nev, int* nex, int* m, int* n, double* H, int* ldh,
                                struct chase_hip_grid* grid, int* init);
void pzchase_init_hip_(int* N, int* nev, int* nex, int* m, int* n, void* H, int* ldh, void* V, double* ritzv,
                       struct chase_hip_grid* grid, int* init);
void pzchase_init_internal_hip_(int* N, int* nev, int* nex, int* m, int* n, void* H, int* ldh,
                                struct chase_hip_grid* grid, int* init);
void pzchase_init_pseudo_hip_(int* N, int* nev, int* nex, int* m, int* n, void* H, int* ldh, void* V, double* ritzv,
                              struct chase_hip_grid* grid, int* init);
void pzchase_init_pseudo_internal_hip_(int* N, int* nev, int* nex, int* m, int* n, void* H, int* ldh,
                                       struct chase_hip_grid* grid, int* init);
void pdchase_init_blockcyclic_hip_(int* N, int* nev, int* nex, int* mbsize, int* nbsize, double* H, int* ldh, double* V,
                                   double* ritzv, int* irsrc, int* icsrc, struct chase_hip_grid* grid, int* init);
void pdchase_init_blockcyclic_internal_hip_(int* N, int* nev, int* nex, int* mbsize, int* nbsize, double* H, int* ldh,
                                            int* irsrc, int* icsrc, struct chase_hip_grid* grid, int* init);
void pzchase_init_blockcyclic_hip_(int* N, int* nev, int* nex, int* mbsize, int* nbsize, void* H, int* ldh, void* V,
                                   double* ritzv, int* irsrc, int* icsrc, struct chase_hip_grid* grid, int* init);
void pzchase_init_blockcyclic_internal_hip_(int* N, int* nev, int* nex, int* mbsize, int* nbsize, void* H, int* ldh,
                                            int* irsrc, int* icsrc, struct chase_hip_grid* grid, int* init);
void pzchase_init_pseudo_blockcyclic_hip_(int* N, int* nev, int* nex, int* mbsize, int* nbsize, void* H, int* ldh, void* V,
                                          double* ritzv, int* irsrc, int* icsrc, struct chase_hip_grid* grid, int* init);
void pzchase_init_pseudo_blockcyclic_internal_hip_(int* N, int* nev, int* nex, int* mbsize, int* nbsize, void* H, int* ldh,
                                                   int* irsrc, int* icsrc, struct chase_hip_grid* grid, int* init);
void pdchase_(int* deg, double* tol, char* mode, char* opt, char* qr);
void pzchase_(int* deg, double* tol, char* mode, char* opt, char* qr);
void pdchase_get_eigenpairs_(double* LEigsV, int* ld, double* ritzv);
void pzchase_get_eigenpairs_(void* LEigsV, int* ld, double* ritzv);
void pdchase_finalize_(int* flag);
void pzchase_finalize_(int* flag);
void pdchase_readHam_(const char* filename);
void pzchase_readHam_(const char* filename);
void pdchase_wrtHam_(const char* filename);
void pzchase_wrtHam_(const char* filename);
#ifdef __cplusplus
}
#endif
#endif
