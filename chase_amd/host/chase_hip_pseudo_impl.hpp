// chase_hip_pseudo_impl.hpp — ChaseHipPseudo<T, BaseT>: single-MI355X Impl of the ChaseBase<T> surface for
// pseudo-Hermitian (Bethe-Salpeter) matrices  H = [[A, B], [-conj(B), -conj(A)]],  S H Hermitian, S = diag(I, -I).
//
// Mirrors ChASECPU<T, PseudoHermitianMatrix<T>> / ChASEGPU<T, PseudoHermitianMatrix<T, GPU>> virtual by virtual:
//   constructor, initVecs       Impl/chase_cpu/chase_cpu.hpp:78-97,296-327        (2*(nev+nex) columns, lower rows x 0.001)
//   HEMM_H2                     Impl/chase_cpu/chase_cpu.hpp:510-555               (Vec2 = alpha H (H Vec1) + beta Vec2 + gamma Vec1)
//   ApplyKconjugate             Impl/chase_cpu/chase_cpu.hpp:557-588               (second half = K-conjugate of the first)
//   QR (S-orthogonal locking)   Impl/chase_cpu/chase_cpu.hpp:590-776
//   RR -> rayleighRitz_v2       linalg/internal/cpu/rayleighRitz.hpp:285-392
//   Resd                        Impl/chase_cpu/chase_cpu.hpp:805-818
//   Lanczos (S inner product)   linalg/internal/cpu/lanczos.hpp:302-470
// Everything that is plumbing of the sequential Impl (getters, life cycle, filter timing, deferred Swap, ReinitColumns,
// LanczosDos, recompute_residuals, the CholQR / Householder choice, allocation) is inherited from ChaseHip with a vector
// block of 2*(nev+nex) columns; its Hermitian-only state (cached H V, residual re-check, the mixed_precision switch and its
// bf16x3 products) is never switched on.
// Mixed precision has a key of its own here, h2_mixed_precision / CHASE_HIP_H2_MIXED_PRECISION=1, default off (the reference's
// CHASE_ENABLE_MIXED_PRECISION does nothing for pseudo-Hermitian matrices): an H^2 filter call that starts while the smallest
// residual of the unlocked wanted pairs is above 1e-3 runs its steps in fp32 on the inherited shadows.  H^2 carries its shift in
// gamma, so H never moves: its shadow is converted once per resident matrix.  Only the unlocked first-half columns enter fp32.
// Column layout of the vector block: [locked | first half (unconverged) | second half (unconverged) | locked].
// All O(N n) / O(N^2 n) work runs in the gfx950 kernels through the C ABI; the (2 nevex)^2 dense core of the
// Rayleigh-Ritz step (potrf, three trsm, heevd) runs on the host like the reference CPU path.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <random>
#include <vector>
#include "chase_hip_impl.hpp"

namespace chase_amd {

template <class T, class BaseT = ChaseBase<T>, class ConfigT = ChaseConfig<T>>
class ChaseHipPseudo : public ChaseHip<T, BaseT, ConfigT> {
    using P = ChaseHip<T, BaseT, ConfigT>;
    using P::ctx_; using P::N_; using P::nevex_; using P::nc_; using P::locked_; using P::resid_;
    using P::dH_; using P::ldd_h_; using P::dV1_; using P::dV2_; using P::dA_; using P::dScal_;
    using P::lanczosIter_; using P::numLanczos_; using P::hemm_calls_;
    using P::gemm; using P::flush_swaps; using P::qr_block;
    using P::nev_; using P::sH_; using P::sV1_; using P::sV2_; using P::ld_s_; using P::hs_valid_; using P::h_resident_;
    using P::sp_active_; using P::sp_synced_; using P::hemm_sp_calls_; using P::hemm_sp_vecs_; using P::sp_filters_;
    using P::gemm32; using P::upload_H; using P::shadow_ld;
public:
    using R = Base<T>;
    using ST = typename P::ST;
    using P::CP;
    static constexpr int E = CP ? 2 : 1;

    // H: N x N (ldh), V1: N x 2*(nev+nex) (ldv), ritzv: 2*(nev+nex) reals — the reference's pseudo constructor contract
    ChaseHipPseudo(chase_hip_ctx* ctx, std::size_t N, std::size_t nev, std::size_t nex, T* H, std::size_t ldh, T* V1,
                   std::size_t ldv, R* ritzv, bool h_on_device = false)
        : P(checked(ctx, N, nev, nex, ldh, ldv), N, nev, nex, H, ldh, V1, ldv, ritzv, h_on_device, 2 * (nev + nex),
            3 * (2 * (nev + nex)) * (2 * (nev + nex)))                    // dA_: 3 nc^2 for the projected matrices of RR
    {
        this->alloc((void**)&dTmp_, N_ * nc_ * sizeof(T));
        this->mixed_ = false;                                             // the H^2 filter runs in fp64
        mixed_precision_env_ignored("the pseudo-Hermitian solver");
        this->sp_split_ = false;
        sp_product_env_ignored("the pseudo-Hermitian solver");
        this->sp_prepack_ = false;
        sp_prepack_env_ignored("the pseudo-Hermitian solver");
        h2_mixed_ = h2_mixed_precision_env() != 0;
    }

    bool set_mixed_precision(bool on) override { return !on; }
    bool set_sp_product(int v) override { return v == 0; }
    bool set_sp_prepack(int v) override { return v == 0; }
    bool set_h2_mixed_precision(bool on) override { h2_mixed_ = on; return true; }
    bool h2_mixed_precision() const override { return h2_mixed_; }
    std::size_t sp_h_converts() const override { return sp_h_converts_; }
    void reset_counters() override { P::reset_counters(); sp_h_converts_ = 0; }
    bool isSym() override { return false; }
    bool isPseudoHerm() override { return true; }
    bool checkSymmetryEasy() override { return false; }
    bool checkPseudoHermicityEasy() override { return true; }
    void symOrHermMatrix(char) override {}
    void Shift(T, bool = false) override {}                   // the H^2 filter carries the shift in gamma
    void HEMM(std::size_t, T, T, std::size_t, std::size_t = 0) override
    {
        throw std::logic_error("ChaseHipPseudo: the pseudo-Hermitian filter uses HEMM_H2");
    }

    // The filter call's bracket: the mixed-precision decision is taken at its start, once per call, from the residuals the driver
    // left in resid_ (all max() before the first iteration) - the Hermitian Impl's rule, which decides in Shift
    void FilterPhaseStart() override
    {
        P::FilterPhaseStart();
        if (h2_mixed_ && locked_ < nev_ && *std::min_element(resid_.begin() + locked_, resid_.begin() + nev_) > (R)1e-3)
            h2_begin_single_precision();
    }
    void FilterPhaseEnd() override
    {
        if (sp_active_) h2_end_single_precision();               // inside the timed phase: the conversions are filter time
        P::FilterPhaseEnd();
    }

    void HEMM_H2(std::size_t block, T alpha, T beta, T gamma, std::size_t offset_left, std::size_t offset_right = 0) override
    {
        flush_swaps();
        std::size_t ncols = (offset_right < block) ? block - offset_right : 0;
        if (ncols != 0) {
            const std::size_t c0 = offset_left + locked_;
            // the reference's filter call runs `block` columns from c0, i.e. past the first half into second-half columns
            // that ApplyKconjugate overwrites right after the filter (algorithm.inc:1012-1064): stop at the first half
            if (c0 >= nevex_) { swap_buffers(); return; }
            if (c0 + ncols > nevex_) ncols = nevex_ - c0;
            if (sp_active_) {
                h2_step_single_precision(c0, ncols, alpha, beta, gamma);
            } else {
                T* v1 = dV1_ + c0 * N_;
                T* v2 = dV2_ + c0 * N_;
                gemm('N', N_, ncols, N_, T(1), dH_, ldd_h_, v1, N_, T(0), dTmp_, N_);
                gemm('N', N_, ncols, N_, alpha, dH_, ldd_h_, dTmp_, N_, beta, v2, N_);
                upload_scalar(gamma);
                hip_ok(chase_hip_col_axpy(ctx_, CP, (int)N_, (int)ncols, (const double*)dScal_, 0, 0, 1.0, v1, (long)N_, v2,
                                          (long)N_), "axpy gamma");
                hemm_calls_ += 2;
            }
        }
        swap_buffers();
    }

    void ApplyKconjugate(std::size_t block) override
    {
        CHASE_PHASE(ctx_, "ApplyKconjugate");
        flush_swaps();
        const std::size_t h = N_ / 2, c2 = nc_ - locked_ - block;
        T* first = dV1_ + locked_ * N_;
        T* second = dV1_ + c2 * N_;
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)h, (int)block, first, (long)N_, second + h, (long)N_), "lacpy");
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)h, (int)block, first + h, (long)N_, second, (long)N_), "lacpy");
        if (CP) hip_ok(chase_hip_conj(ctx_, (int)N_, (int)block, second, (long)N_), "conj");
    }

    void QR(std::size_t, R cond) override
    {
        CHASE_PHASE(ctx_, "QR");
        flush_swaps();
        const std::size_t L = locked_;
        const int n = (int)N_;
        lacpy(L, dV1_, dV2_);                                            // V2[:, :L] = V1[:, :L]
        lacpy(L, dV1_ + (nc_ - L) * N_, dV2_ + L * N_);                  // V2[:, L:2L] = V1[:, nc-L:]
        lacpy(nc_ - 2 * L, dV1_ + L * N_, dV2_ + 2 * L * N_);            // V2[:, 2L:] = active block
        std::swap(dV1_, dV2_);
        // S-orthogonalise against the locked vectors: flip the lower half of the 2L locked columns
        hip_ok(chase_hip_scale_rows(ctx_, CP, n, (int)(2 * L), dV1_, (long)N_, (int)(N_ / 2), -1.0), "flip");
        qr_block(cond);
        lacpy(nc_ - 2 * L, dV1_ + 2 * L * N_, dV2_ + L * N_);            // active block back to the middle of V2
        std::swap(dV1_, dV2_);
        lacpy(L, dV1_, dV2_);
        lacpy(L, dV1_ + (nc_ - L) * N_, dV2_ + (nc_ - L) * N_);
    }

    void RR(R* ritzv, std::size_t block) override
    {
        CHASE_PHASE(ctx_, "RR");
        flush_swaps();
        const std::size_t n = 2 * block, k = N_ / 2;
        T* Q = dV1_ + locked_ * N_;
        T* W = dV2_ + locked_ * N_;
        T* A = dA_;
        T* M = dA_ + n * n;
        chase_hip_ctx_set_phase(ctx_, 2);
        gemm('N', N_, n, N_, T(1), dH_, ldd_h_, Q, N_, T(0), W, N_);                      // W = H Q
        chase_hip_ctx_set_phase(ctx_, 0);
        hip_ok(chase_hip_scale_rows(ctx_, CP, (int)N_, (int)n, W, (long)N_, (int)k, -1.0), "flip");   // W = S H Q
        gemm('C', n, n, N_, T(1), Q, N_, W, N_, T(0), A, n);                              // A = Q^H S H Q
        hip_ok(chase_hip_set_identity(ctx_, CP, (int)n, M, (long)n), "identity");
        gemm('C', n, n, k, T(-2), Q + k, N_, Q + k, N_, T(1), M, n);                     // M = I - 2 Q2^H Q2
        const int info = chase_hip_pseudo_rr_small(ctx_, CP, (int)n, A, M, ritzv);
        if (info > 0) throw std::runtime_error("ChaseHipPseudo::RR: Q^H S H Q is not positive definite (potrf info " +
                                               std::to_string(info) + ")");
        hip_ok(info, "pseudo_rr_small");
        gemm('N', N_, n / 2, n, T(1), Q, N_, M, n, T(0), W, N_);                          // first n/2 Ritz vectors
        std::swap(dV1_, dV2_);
    }

    void Resd(R* ritzv, R* resd, std::size_t) override
    {
        CHASE_PHASE(ctx_, "Resd");
        flush_swaps();
        const std::size_t sub = nevex_ - locked_;
        T* V = dV1_ + locked_ * N_;
        T* W = dV2_ + locked_ * N_;
        chase_hip_ctx_set_phase(ctx_, 3);                     // the residuals the convergence test reads: four products
        gemm('N', N_, sub, N_, T(1), dH_, ldd_h_, V, N_, T(0), W, N_);
        chase_hip_ctx_set_phase(ctx_, 0);
        hip_ok(chase_hip_resid_norms(ctx_, CP, (int)N_, (int)sub, W, (long)N_, V, (long)N_, ritzv, resd, 0), "resid");
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
    // chase_cpu.hpp:310-321: damp the lower block of random start vectors
    void init_vecs_hook(bool random) override
    {
        if (random)
            hip_ok(chase_hip_scale_rows(ctx_, CP, (int)N_, (int)nc_, dV1_, (long)N_, (int)(N_ / 2), 0.001), "scale_rows");
    }
    T* swap_scratch() override { return dTmp_; }

private:
    // the constructor's argument checks, run before the base class allocates anything
    static chase_hip_ctx* checked(chase_hip_ctx* ctx, std::size_t N, std::size_t nev, std::size_t nex, std::size_t ldh,
                                  std::size_t ldv)
    {
        if (!ctx) throw std::invalid_argument("ChaseHipPseudo: null context");
        if (N == 0 || nev + nex == 0 || 2 * (nev + nex) > N) throw std::invalid_argument("ChaseHipPseudo: need 0 < 2(nev+nex) <= N");
        if (N % 2) throw std::invalid_argument("ChaseHipPseudo: N must be even (2 x 2 block structure)");
        if (ldh < N || ldv < N) throw std::invalid_argument("ChaseHipPseudo: leading dimension smaller than N");
        return ctx;
    }
    void swap_buffers()
    {
        std::swap(dV1_, dV2_);
        if (sp_active_) std::swap(sV1_, sV2_);                // the shadows follow their buffers
    }
    // a qualifying filter call: shadows of the first half's nevex_ columns, allocated on first use, and fp32(H) - converted once
    // per resident matrix (upload_H invalidates it); there is no shift to follow
    void h2_begin_single_precision()
    {
        if (!sV1_) {
            ld_s_ = shadow_ld(N_);
            this->alloc((void**)&sV1_, ld_s_ * nevex_ * sizeof(ST));
            this->alloc((void**)&sV2_, ld_s_ * nevex_ * sizeof(ST));
            this->alloc((void**)&sTmp_, ld_s_ * nevex_ * sizeof(ST));
            this->alloc((void**)&sH_, ld_s_ * N_ * sizeof(ST));
        }
        if (!h_resident_) upload_H();
        if (!hs_valid_) {
            hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)N_, (int)N_, dH_, (long)ldd_h_, sH_, (long)ld_s_), "convert_d2s H");
            hs_valid_ = true;
            ++sp_h_converts_;
        }
        sp_active_ = true;
        sp_synced_ = false;
    }
    // V2 = alpha H (H V1) + beta V2 + gamma V1 on the shadows, columns [c0, c0 + ncols) of the first half
    void h2_step_single_precision(std::size_t c0, std::size_t ncols, T alpha, T beta, T gamma)
    {
        if (!sp_synced_) {
            // the vectors enter fp32 right before the first fp32 product: unlocked first-half columns of both buffers
            const std::size_t sub = nevex_ - locked_;
            hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)N_, (int)sub, dV1_ + locked_ * N_, (long)N_, sV1_ + locked_ * ld_s_,
                                         (long)ld_s_), "convert_d2s");
            hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)N_, (int)sub, dV2_ + locked_ * N_, (long)N_, sV2_ + locked_ * ld_s_,
                                         (long)ld_s_), "convert_d2s");
            sp_synced_ = true;
            ++sp_filters_;
        }
        ST* v1 = sV1_ + c0 * ld_s_;
        ST* v2 = sV2_ + c0 * ld_s_;
        ST* tmp = sTmp_ + c0 * ld_s_;
        gemm32(N_, ncols, N_, T(1), sH_, ld_s_, v1, ld_s_, T(0), tmp, ld_s_);
        gemm32(N_, ncols, N_, alpha, sH_, ld_s_, tmp, ld_s_, beta, v2, ld_s_);
        const float g[2] = {(float)std::real(gamma), (float)std::imag(gamma)};
        hip_ok(chase_hip_axpy_sp(ctx_, CP, (int)N_, (int)ncols, g, v1, (long)ld_s_, v2, (long)ld_s_), "axpy_sp gamma");
        hemm_sp_calls_ += 2;
        hemm_sp_vecs_ += 2 * ncols;
    }
    // the end of the call: the filtered (unlocked first-half) columns return to fp64; locked columns and the second half -
    // which ApplyKconjugate rebuilds in fp64 right after - were never touched
    void h2_end_single_precision()
    {
        if (sp_synced_)
            hip_ok(chase_hip_convert_s2d(ctx_, CP, (int)N_, (int)(nevex_ - locked_), sV1_ + locked_ * ld_s_, (long)ld_s_,
                                         dV1_ + locked_ * N_, (long)N_), "convert_s2d");
        sp_active_ = false;
        sp_synced_ = false;
    }
    void lacpy(std::size_t ncols, const T* src, T* dst)
    {
        if (ncols) hip_ok(chase_hip_lacpy(ctx_, CP, (int)N_, (int)ncols, src, (long)N_, dst, (long)N_), "lacpy");
    }
    void upload_scalar(T v)
    {
        double h[2] = {std::real(v), CP ? std::imag(v) : 0.0};
        hip_ok(chase_hip_memcpy_h2d(ctx_, dScal_, h, sizeof h), "h2d");
    }

    // S-inner-product Lanczos (cpu/lanczos.hpp:302-470).  The per-step scalars go through the host: M <= 50 steps of
    // numvec <= 16 vectors, the products and updates stay on the device.
    void lanczos_core(std::size_t M, std::size_t nv, bool store, R* theta, R* Tau, R* ritzV)
    {
        flush_swaps();
        using C = std::complex<double>;
        T *v0, *v1, *v2, *Sv;
        double* dsc;
        void* blk = nullptr;
        const std::size_t vb = 4 * N_ * nv * sizeof(T), sb = 8 * nv * sizeof(double);
        int rc = chase_hip_malloc(ctx_, &blk, vb + sb);
        if (rc) throw HipStatusError(rc, "lanczos workspace");
        v0 = (T*)blk; v1 = v0 + N_ * nv; v2 = v1 + N_ * nv; Sv = v2 + N_ * nv;
        dsc = (double*)(Sv + N_ * nv);
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
        auto scal = [&](const std::vector<C>& a, T* x) {                         // x_i *= a_i (complex scale via axpy on zeroed copy)
            // x <- a x  ==  x += (a - 1) x
            std::vector<C> am(nv);
            for (std::size_t i = 0; i < nv; ++i) am[i] = a[i] - C(1, 0);
            hip_ok(chase_hip_lacpy(ctx_, CP, n, nvi, x, (long)N_, dTmp_, (long)N_), "lacpy");
            axpy(am, dTmp_, x);
        };
        auto hv = [&]() {                                                        // v2 = H v1 ; Sv = S v2
            gemm('N', N_, nv, N_, T(1), dH_, ldd_h_, v1, N_, T(0), v2, N_);
            hip_ok(chase_hip_lacpy(ctx_, CP, n, nvi, v2, (long)N_, Sv, (long)N_), "lacpy");
            hip_ok(chase_hip_scale_rows(ctx_, CP, n, nvi, Sv, (long)N_, (int)(N_ / 2), -1.0), "flip");
        };
        try {
            hip_ok(chase_hip_memset(ctx_, blk, 0, vb + sb), "memset");
            hip_ok(chase_hip_lacpy(ctx_, CP, n, nvi, dV1_, (long)N_, v1, (long)N_), "lacpy");
            std::vector<C> alpha(nv), beta(nv);
            std::vector<double> d(M * nv, 0.0), e(M * nv, 0.0);
            hv();
            dots(v1, Sv, beta);
            for (auto& b : beta) b = C(1, 0) / std::sqrt(b);
            scal(beta, v1); scal(beta, v2);
            for (std::size_t k = 0; k < M; ++k) {
                if (store)
                    hip_ok(chase_hip_lacpy(ctx_, CP, n, 1, v1 + (nv - 1) * N_, (long)N_, dV1_ + k * N_, (long)N_), "lacpy");
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
            if (store) hip_ok(chase_hip_lacpy(ctx_, CP, n, nvi, v1, (long)N_, dV1_, (long)N_), "lacpy");
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

    T* dTmp_ = nullptr;                   // N x nc scratch: H V1 of the H^2 filter, deferred swaps, Lanczos scaling
    bool h2_mixed_ = false;               // h2_mixed_precision
    ST* sTmp_ = nullptr;                  // ld_s_ x nevex_: H V1 of an fp32 H^2 step
    std::size_t sp_h_converts_ = 0;       // whole-matrix conversions of H into sH_
};

} // namespace chase_amd
