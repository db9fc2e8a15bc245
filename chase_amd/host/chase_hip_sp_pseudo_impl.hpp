// chase_hip_sp_pseudo_impl.hpp — ChaseHipSpPseudo<T, BaseT>: the single-precision pseudo-Hermitian (Bethe-Salpeter) solver on one
// MI355X (the reference's ChASEGPU<std::complex<float>, PseudoHermitianMatrix<...>> and its real twin; cchase_pseudo_).
//
// ChaseHipPseudo's algorithm with ChaseHipSp's precision rules.  T is double / std::complex<double>: the driver (Solve_pseudo), Ritz
// values, residuals and scalars are fp64 on the host.  The DATA are fp32 from start to end: H (N x N, used in place at its ld when
// it already lives in HBM), V1 and V2 (N x nc, nc = 2 (nev+nex), columns [locked | first half | second half | locked]) and an
// N x (nev+nex) scratch for H V1.  No fp64 copy of H ever exists on the device.
//
//   initVecs         the host mt19937(1337) normals of all nc columns rounded to fp32; lower N/2 rows times fl32(0.001) on the device
//   HEMM_H2          tmp = H v1, v2 = alpha H tmp + beta v2 (chase_hip_gemm_s / _c), v2 += gamma v1 (chase_hip_axpy_sp); first half only
//   ApplyKconjugate  one chase_hip_kconj_sp launch
//   QR               ChaseHipPseudo's column shuffle in fp32; all nc columns widened, the 2L locked ones flipped there (S-orthogonality),
//                    CholQR / Householder in fp64 with the float thresholds, rounded back; locked columns keep their fp32 bits
//   RR               W = S (H Q) in fp32 (the flip is exact), A = Q^H W and M = I - 2 Q2^H Q2 accumulated into fp64, the dense core
//                    chase_hip_pseudo_rr_small in fp64, the first n/2 eigenvector columns rounded, V = Q M32 in fp32
//   Resd             W = H V in fp32, chase_hip_resid_norms_sp
//   Lanczos          the S-inner-product recurrence on fp64 vectors in the scratch; each H v is convert_d2s + gemm_sd / _cz
// Getters, life cycle, filter timing, deferred Swap, Lock, ReinitColumns, LanczosDos, End, recompute_residuals, peek_widened and
// device_bytes are ChaseHipSp's at width nc.  There is no mixed_precision / sp_product / sp_prepack / h2_mixed_precision here (every
// product is the fp32 MFMA one), no tape and no device_rng.
#pragma once
#include "chase_hip_sp_impl.hpp"

namespace chase_amd {

template <class T, class BaseT = ChaseBase<T>, class ConfigT = ChaseConfig<T>>
class ChaseHipSpPseudo : public ChaseHipSp<T, BaseT, ConfigT> {
    using P = ChaseHipSp<T, BaseT, ConfigT>;
    using P::ctx_; using P::N_; using P::nevex_; using P::nc_; using P::locked_; using P::resid_; using P::ld_;
    using P::dH_; using P::ldd_h_; using P::dV1_; using P::dV2_; using P::dW_; using P::w_cols_; using P::dA_; using P::dAs_;
    using P::lanczosIter_; using P::numLanczos_; using P::hemm_sp_calls_; using P::hemm_sp_vecs_; using P::h_resident_;
    using P::gemm32; using P::gemm32w; using P::flush_swaps; using P::qr_block; using P::upload_H;
public:
    using R = Base<T>;
    using ST = typename P::ST;
    using P::CP;
    static constexpr int E = CP ? 2 : 1;

    // H: N x N fp32 (ldh), V1: N x 2*(nev+nex) fp32 (ldv), ritzv: 2*(nev+nex) doubles - ChaseHipPseudo's contract on fp32 data
    ChaseHipSpPseudo(chase_hip_ctx* ctx, std::size_t N, std::size_t nev, std::size_t nex, ST* H, std::size_t ldh, ST* V1,
                     std::size_t ldv, R* ritzv, bool h_on_device = false)
        : P(checked(ctx, N, nev, nex, ldh, ldv), N, nev, nex, H, ldh, V1, ldv, ritzv, h_on_device, 2 * (nev + nex),
            2 * (2 * (nev + nex)) * (2 * (nev + nex)))                    // dA_: the two projected matrices of RR
    {
        this->alloc((void**)&sTmp_, ld_ * nevex_ * sizeof(ST));
    }

    bool isSym() override { return false; }
    bool isPseudoHerm() override { return true; }
    bool checkSymmetryEasy() override { return false; }
    bool checkPseudoHermicityEasy() override { return true; }
    void symOrHermMatrix(char) override {}
    void Shift(T, bool = false) override {}                   // the H^2 filter carries the shift in gamma
    void HEMM(std::size_t, T, T, std::size_t, std::size_t = 0) override
    {
        throw std::logic_error("ChaseHipSpPseudo: the pseudo-Hermitian filter uses HEMM_H2");
    }

    void HEMM_H2(std::size_t block, T alpha, T beta, T gamma, std::size_t offset_left, std::size_t offset_right = 0) override
    {
        flush_swaps();
        std::size_t ncols = (offset_right < block) ? block - offset_right : 0;
        if (ncols != 0) {
            const std::size_t c0 = offset_left + locked_;
            // as ChaseHipPseudo::HEMM_H2: the second half is rebuilt by ApplyKconjugate right after the filter - stop at the first
            if (c0 >= nevex_) { std::swap(dV1_, dV2_); return; }
            if (c0 + ncols > nevex_) ncols = nevex_ - c0;
            if (!h_resident_) upload_H();
            ST* v1 = dV1_ + c0 * ld_;
            ST* v2 = dV2_ + c0 * ld_;
            ST* tmp = sTmp_ + c0 * ld_;
            gemm32(N_, ncols, N_, T(1), dH_, ldd_h_, v1, ld_, T(0), tmp, ld_);
            gemm32(N_, ncols, N_, alpha, dH_, ldd_h_, tmp, ld_, beta, v2, ld_);
            const float g[2] = {(float)std::real(gamma), (float)std::imag(gamma)};
            hip_ok(chase_hip_axpy_sp(ctx_, CP, (int)N_, (int)ncols, g, v1, (long)ld_, v2, (long)ld_), "axpy_sp gamma");
            hemm_sp_calls_ += 2;
            hemm_sp_vecs_ += 2 * ncols;
        }
        std::swap(dV1_, dV2_);
    }

    void ApplyKconjugate(std::size_t block) override
    {
        CHASE_PHASE(ctx_, "ApplyKconjugate");
        flush_swaps();
        if (2 * (locked_ + block) > nc_) throw std::invalid_argument("ApplyKconjugate: columns beyond the first half");
        const std::size_t c2 = nc_ - locked_ - block;
        hip_ok(chase_hip_kconj_sp(ctx_, CP, (int)N_, (int)block, dV1_ + locked_ * ld_, (long)ld_, dV1_ + c2 * ld_, (long)ld_), "kconj_sp");
    }

    void QR(std::size_t, R cond) override
    {
        CHASE_PHASE(ctx_, "QR");
        flush_swaps();
        const std::size_t L = locked_;
        lacpy(L, dV1_, dV2_);                                            // V2[:, :L] = V1[:, :L]
        lacpy(L, dV1_ + (nc_ - L) * ld_, dV2_ + L * ld_);                // V2[:, L:2L] = V1[:, nc-L:]
        lacpy(nc_ - 2 * L, dV1_ + L * ld_, dV2_ + 2 * L * ld_);          // V2[:, 2L:] = active block
        std::swap(dV1_, dV2_);
        qr_block(cond);                                                  // (qr_widened_hook flips the 2L locked columns in fp64)
        lacpy(nc_ - 2 * L, dV1_ + 2 * L * ld_, dV2_ + L * ld_);          // active block back to the middle of V2
        std::swap(dV1_, dV2_);                                           // the locked columns here are the saved fp32 ones
        lacpy(L, dV1_, dV2_);
        lacpy(L, dV1_ + (nc_ - L) * ld_, dV2_ + (nc_ - L) * ld_);
    }

    void RR(R* ritzv, std::size_t block) override
    {
        CHASE_PHASE(ctx_, "RR");
        flush_swaps();
        if (locked_ + 2 * block > nc_) throw std::invalid_argument("RR: columns beyond the block");
        if (!h_resident_) upload_H();
        const std::size_t n = 2 * block, k = N_ / 2;
        ST* Q = dV1_ + locked_ * ld_;
        ST* W = dV2_ + locked_ * ld_;
        T* A = dA_;
        T* M = dA_ + n * n;
        gemm32(N_, n, N_, T(1), dH_, ldd_h_, Q, ld_, T(0), W, ld_);                                        // W = H Q
        hip_ok(chase_hip_scale_rows_sp(ctx_, CP, (int)N_, (int)n, W, (long)ld_, (int)k, -1.0f), "flip");  // W = S H Q (exact)
        gemm32w('C', n, n, N_, Q, ld_, W, ld_, A, n);                                                      // A = Q^H S H Q in fp64
        hip_ok(chase_hip_set_identity(ctx_, CP, (int)n, M, (long)n), "identity");
        gemm32w('C', n, n, k, Q + k, ld_, Q + k, ld_, M, n, -2.0, 1.0);                                    // M = I - 2 Q2^H Q2
        const int info = chase_hip_pseudo_rr_small(ctx_, CP, (int)n, A, M, ritzv);
        if (info > 0) throw std::runtime_error("ChaseHipSpPseudo::RR: Q^H S H Q is not positive definite (potrf info " +
                                               std::to_string(info) + ")");
        hip_ok(info, "pseudo_rr_small");
        hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)n, (int)(n / 2), M, (long)n, dAs_, (long)n), "convert_d2s");
        gemm32(N_, n / 2, n, T(1), Q, ld_, dAs_, n, T(0), W, ld_);                                         // first n/2 Ritz vectors
        std::swap(dV1_, dV2_);
    }

    void Resd(R* ritzv, R* resd, std::size_t) override
    {
        CHASE_PHASE(ctx_, "Resd");
        flush_swaps();
        if (!h_resident_) upload_H();
        const std::size_t sub = nevex_ - locked_;
        ST* V = dV1_ + locked_ * ld_;
        ST* W = dV2_ + locked_ * ld_;
        gemm32(N_, sub, N_, T(1), dH_, ldd_h_, V, ld_, T(0), W, ld_);
        hip_ok(chase_hip_resid_norms_sp(ctx_, CP, (int)N_, (int)sub, W, (long)ld_, V, (long)ld_, ritzv, resd), "resid_norms_sp");
        if (resd != resid_.data() + locked_) std::memcpy(resid_.data() + locked_, resd, sub * sizeof(R));
    }

    void Lanczos(std::size_t m, R* upperb) override
    {
        CHASE_PHASE(ctx_, "Lanczos");
        lanczosIter_ = m; numLanczos_ = 1;
        std::vector<R> theta(m), tau(m), z(m * m);
        lanczos_core(m, 1, false, theta.data(), tau.data(), z.data());
        if (upperb) *upperb = theta[m - 1];                   // cpu/lanczos.hpp:629: largest Ritz value of the run
    }
    void Lanczos(std::size_t M, std::size_t numvec, R* upperb, R* ritzv, R* Tau, R* ritzV) override
    {
        CHASE_PHASE(ctx_, "Lanczos");
        lanczosIter_ = M; numLanczos_ = numvec;
        lanczos_core(M, numvec, true, ritzv, Tau, ritzV);
        if (upperb) *upperb = ritzv[M - 1];                   // cpu/lanczos.hpp:515
    }

protected:
    // chase_cpu.hpp:310-321: damp the lower block of random start vectors, one fp32 multiply per component
    void init_vecs_hook(bool random) override
    {
        if (random)
            hip_ok(chase_hip_scale_rows_sp(ctx_, CP, (int)N_, (int)nc_, dV1_, (long)ld_, (int)(N_ / 2), 0.001f), "scale_rows_sp");
    }
    // S-orthogonalise against the locked vectors: flip the lower half of the 2L locked columns of the widened block
    void qr_widened_hook() override
    {
        hip_ok(chase_hip_scale_rows(ctx_, CP, (int)N_, (int)(2 * locked_), dW_, (long)N_, (int)(N_ / 2), -1.0), "flip");
    }

private:
    // the constructor's argument checks, run before the base class allocates anything
    static chase_hip_ctx* checked(chase_hip_ctx* ctx, std::size_t N, std::size_t nev, std::size_t nex, std::size_t ldh,
                                  std::size_t ldv)
    {
        if (!ctx) throw std::invalid_argument("ChaseHipSpPseudo: null context");
        if (N == 0 || nev + nex == 0 || 2 * (nev + nex) > N) throw std::invalid_argument("ChaseHipSpPseudo: need 0 < 2(nev+nex) <= N");
        if (N % 2) throw std::invalid_argument("ChaseHipSpPseudo: N must be even (2 x 2 block structure)");
        if (ldh < N || ldv < N) throw std::invalid_argument("ChaseHipSpPseudo: leading dimension smaller than N");
        return ctx;
    }
    void lacpy(std::size_t ncols, const ST* src, ST* dst)
    {
        if (ncols) hip_ok(chase_hip_lacpy_sp(ctx_, CP, (int)N_, (int)ncols, src, (long)ld_, dst, (long)ld_), "lacpy_sp");
    }
    // C64 = alpha op(A32) B32 + beta C64 with real scalars
    void gemm32w(char op, std::size_t m, std::size_t n, std::size_t k, const ST* A, std::size_t lda, const ST* B, std::size_t ldb, T* C,
                 std::size_t ldc, double alpha, double beta)
    {
        int rc;
        if constexpr (is_cplx<T>::value) {
            const double a[2] = {alpha, 0.0}, b[2] = {beta, 0.0};
            rc = chase_hip_gemm_cz(ctx_, op, (int)m, (int)n, (int)k, a, A, (long)lda, B, (long)ldb, b, C, (long)ldc);
        } else {
            rc = chase_hip_gemm_sd(ctx_, op, (int)m, (int)n, (int)k, alpha, A, (long)lda, B, (long)ldb, beta, C, (long)ldc);
        }
        hip_ok(rc, "gemm32w");
    }

    // S-inner-product Lanczos (cpu/lanczos.hpp:302-470), ChaseHipPseudo::lanczos_core on five blocks of nv fp64 vectors in the scratch
    // (grown when 5 nv > its columns): v0, v1, v2, S v2 and the copy a scaling goes through.  Each H v rounds the block to fp32
    // (transient ld_ x nv) and multiplies the fp32 matrix into fp64.  The per-step scalars go through the host.
    void lanczos_core(std::size_t M, std::size_t nv, bool store, R* theta, R* Tau, R* ritzV)
    {
        flush_swaps();
        if (!h_resident_) upload_H();
        if (nv == 0 || nv > nc_ || M == 0 || (store && M > nc_))
            throw std::invalid_argument("Lanczos: more vectors or steps than the block holds");
        using C = std::complex<double>;
        if (5 * nv > w_cols_) {
            this->alloc((void**)&dW_, N_ * 5 * nv * sizeof(T));       // (the smaller scratch stays owned until the Impl goes)
            w_cols_ = 5 * nv;
        }
        T *v0 = dW_, *v1 = v0 + N_ * nv, *v2 = v1 + N_ * nv, *Sv = v2 + N_ * nv, *cp = Sv + N_ * nv;
        void* blk = nullptr;
        const std::size_t s_bytes = ld_ * nv * sizeof(ST), sb = 8 * nv * sizeof(double);
        int rc = chase_hip_malloc(ctx_, &blk, s_bytes + sb);
        if (rc) throw HipStatusError(rc, "lanczos workspace");
        ST* s1 = (ST*)blk;
        double* dsc = (double*)((char*)blk + s_bytes);
        const int n = (int)N_, nvi = (int)nv;
        std::vector<double> hd(nv * 2), hc(nv * 2);
        auto dots = [&](const T* x, const T* y, std::vector<C>& out) {          // out[i] = x_i^H y_i
            hip_ok(chase_hip_col_dot(ctx_, CP, n, nvi, x, (long)N_, y, (long)N_, dsc), "dot");
            hip_ok(chase_hip_memcpy_d2h(ctx_, hd.data(), dsc, nv * E * sizeof(double)), "d2h");
            for (std::size_t i = 0; i < nv; ++i) out[i] = CP ? C(hd[2 * i], hd[2 * i + 1]) : C(hd[i], 0);
        };
        auto axpy = [&](const std::vector<C>& a, const T* x, T* y) {             // y_i += a_i x_i
            for (std::size_t i = 0; i < nv; ++i) { if (CP) { hc[2 * i] = a[i].real(); hc[2 * i + 1] = a[i].imag(); } else hc[i] = a[i].real(); }
            hip_ok(chase_hip_memcpy_h2d(ctx_, dsc + 2 * nv, hc.data(), nv * E * sizeof(double)), "h2d");
            hip_ok(chase_hip_col_axpy(ctx_, CP, n, nvi, dsc + 2 * nv, 0, 1, 1.0, x, (long)N_, y, (long)N_), "axpy");
        };
        auto scal = [&](const std::vector<C>& a, T* x) {                         // x <- a x  ==  x += (a - 1) x
            std::vector<C> am(nv);
            for (std::size_t i = 0; i < nv; ++i) am[i] = a[i] - C(1, 0);
            hip_ok(chase_hip_lacpy(ctx_, CP, n, nvi, x, (long)N_, cp, (long)N_), "lacpy");
            axpy(am, cp, x);
        };
        auto hv = [&]() {                                                        // v2 = H fl32(v1) ; Sv = S v2
            hip_ok(chase_hip_convert_d2s(ctx_, CP, n, nvi, v1, (long)N_, s1, (long)ld_), "convert_d2s");
            gemm32w('N', N_, nv, N_, dH_, ldd_h_, s1, ld_, v2, N_);
            hip_ok(chase_hip_lacpy(ctx_, CP, n, nvi, v2, (long)N_, Sv, (long)N_), "lacpy");
            hip_ok(chase_hip_scale_rows(ctx_, CP, n, nvi, Sv, (long)N_, (int)(N_ / 2), -1.0), "flip");
        };
        try {
            hip_ok(chase_hip_memset(ctx_, blk, 0, s_bytes + sb), "memset");
            hip_ok(chase_hip_memset(ctx_, dW_, 0, N_ * 5 * nv * sizeof(T)), "memset");
            hip_ok(chase_hip_convert_s2d(ctx_, CP, n, nvi, dV1_, (long)ld_, v1, (long)N_), "convert_s2d");
            std::vector<C> alpha(nv), beta(nv);
            std::vector<double> d(M * nv, 0.0), e(M * nv, 0.0);
            hv();
            dots(v1, Sv, beta);
            for (auto& b : beta) b = C(1, 0) / std::sqrt(b);
            scal(beta, v1); scal(beta, v2);
            for (std::size_t k = 0; k < M; ++k) {
                if (store)   // the reference writes every run's k-th vector into column k (last run wins)
                    hip_ok(chase_hip_convert_d2s(ctx_, CP, n, 1, v1 + (nv - 1) * N_, (long)N_, dV1_ + k * ld_, (long)ld_), "convert_d2s");
                dots(v2, Sv, alpha);
                for (std::size_t i = 0; i < nv; ++i) alpha[i] = -alpha[i] * beta[i];
                axpy(alpha, v1, v2);
                for (std::size_t i = 0; i < nv; ++i) { alpha[i] = -alpha[i]; d[k + M * i] = alpha[i].real(); }
                if (k == M - 1) break;
                for (auto& b : beta) b = -C(1, 0) / b;
                axpy(beta, v0, v2);
                for (auto& b : beta) b = -b;
                T* t = v0; v0 = v1; v1 = v2; v2 = t;                            // (v0, v1, v2) <- (v1, v2, v0)
                hv();
                dots(v1, Sv, beta);
                for (std::size_t i = 0; i < nv; ++i) { beta[i] = std::sqrt(beta[i]); e[k + M * i] = beta[i].real(); beta[i] = C(1, 0) / beta[i]; }
                scal(beta, v1); scal(beta, v2);
            }
            if (store) hip_ok(chase_hip_convert_d2s(ctx_, CP, n, nvi, v1, (long)N_, dV1_, (long)ld_), "convert_d2s");
            hip_ok(chase_hip_ctx_sync(ctx_), "sync");
            chase_hip_free(ctx_, blk);
            blk = nullptr;
            std::vector<double> dd(M), ee(M), w(M), Z(M * M);
            for (std::size_t i = 0; i < nv; ++i) {
                for (std::size_t k = 0; k < M; ++k) { dd[k] = d[k + M * i]; ee[k] = (k + 1 < M) ? e[k + M * i] : 0.0; }
                hip_ok(chase_hip_stemr_host((int)M, dd.data(), ee.data(), w.data(), Z.data(), (int)M), "stemr");
                for (std::size_t k = 0; k < M; ++k) {
                    theta[k + i * M] = w[k];
                    if (Tau) Tau[k + i * M] = std::abs(Z[k * M]) * std::abs(Z[k * M]);
                }
                if (ritzV) std::memcpy(ritzV, Z.data(), M * M * sizeof(double));
            }
        } catch (...) {
            if (blk) chase_hip_free(ctx_, blk);
            throw;
        }
    }

    ST* sTmp_ = nullptr;                  // ld_ x (nev+nex): H V1 of an H^2 filter step
};

} // namespace chase_amd
