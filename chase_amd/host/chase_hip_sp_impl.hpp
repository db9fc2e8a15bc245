// chase_hip_sp_impl.hpp — ChaseHipSp<T, BaseT>: the single-precision Hermitian solver on one MI355X (the reference's
// ChASEGPU<float> / ChASEGPU<std::complex<float>> instantiations, Impl/chase_gpu/chase_gpu.hpp).
//
// T is double / std::complex<double>: the class implements the ChaseBase<T> surface, so the driver (algorithm.hpp), the handle
// and every chase_hip_op_* entry point work unchanged and the driver's scalars, Ritz values and residuals stay fp64 on the host.
// The DATA are single precision from start to end: the caller's H and V, and H, V1 and V2 on the device, are float /
// complex<float>.  No fp64 copy of H ever exists on the device.
//
//   HEMM     chase_hip_gemm_s / _c (the fp32 MFMA product) on H and the fp32 blocks, every step of every filter call
//   Shift    H_ii = fl32(d0_i + s) from the saved diagonal d0 and the accumulated shift s: fp32 (h + c) - c does not give h back,
//            the reference's in-place shift would let the diagonal drift; the unshift restores the saved bits
//   QR       the reference's default QR_DOUBLE_PRECISION (chase_gpu.hpp:168-180,826-905): all columns widened into an fp64
//            scratch, CholQR / Householder there with the single-precision thresholds 1e4 / 1e1 (chase_gpu.hpp:808-809), rounded back
//   RR       W = H Q in fp32, A = Q^H W accumulated on the f32 matrix cores into fp64, heevd in fp64, eigenvectors rounded, V = Q A
//   Resd     W = H V in fp32, norms of W - lambda V formed and summed in fp64; no reuse of RR's product, no borderline re-check
//   Lanczos  the few Lanczos vectors live in the fp64 scratch (chase_hip_col_* kernels); each H v is convert_d2s + gemm_sd / _cz
//
// It carries none of ChaseHip's fp64 shadows, cached H V, re-check or packing state.  Plugging it into a ChASE checkout as
// ChaseBase<float> is out of scope.
// ChaseHipSpPseudo (chase_hip_sp_pseudo_impl.hpp) derives from it as ChaseHipPseudo does from ChaseHip: the members are protected, the
// vector blocks have nc_ columns (nev+nex here, twice that there), and QR's factorisation is qr_block with a hook on the widened block.
#pragma once
#include "chase_hip_impl.hpp"

namespace chase_amd {

template <class T, class BaseT = ChaseBase<T>, class ConfigT = ChaseConfig<T>>
class ChaseHipSp : public WithOutput<BaseT>, public HipImplExtras {
public:
    using R = Base<T>;
    static constexpr int CP = is_cplx<T>::value ? 1 : 0;
    using ST = std::conditional_t<is_cplx<T>::value, std::complex<float>, float>;      // element of H and the vector blocks

    // H: N x N fp32 column-major (ldh), V1: N x (nev+nex) fp32 (ldv), ritzv: nev+nex doubles.  h_on_device: H already lives in
    // HBM and is used in place at its ld (shifted and unshifted by the filter)
    // ncols / a_elems: the pseudo-Hermitian Impl (chase_hip_sp_pseudo_impl.hpp) holds 2 (nev+nex) columns and two projected matrices
    ChaseHipSp(chase_hip_ctx* ctx, std::size_t N, std::size_t nev, std::size_t nex, ST* H, std::size_t ldh, ST* V1,
               std::size_t ldv, R* ritzv, bool h_on_device = false, std::size_t ncols = 0, std::size_t a_elems = 0)
        : ctx_(ctx), N_(N), nev_(nev), nex_(nex), nevex_(nev + nex), nc_(ncols ? ncols : nev + nex), H_(H), ldh_(ldh), V1_(V1),
          ldv_(ldv), ritzv_(ritzv), h_on_device_(h_on_device), config_(N, nev, nex), resid_(nc_, 0), perm_(nc_)
    {
        if (!ctx) throw std::invalid_argument("ChaseHipSp: null context");
        if (N == 0 || nevex_ == 0 || nc_ > N) throw std::invalid_argument("ChaseHipSp: need 0 < nev+nex <= N");
        if (ldh < N || ldv < N) throw std::invalid_argument("ChaseHipSp: leading dimension smaller than N");
        // the reference's single-precision defaults (algorithm/configuration.hpp:58-129)
        config_.SetTol(1e-5); config_.SetDeg(10); config_.SetMaxDeg(18); config_.SetLanczosIter(12);
        reset_perm();
        ld_ = shadow_ld(N_);
        if (h_on_device_) { dH_ = H; ldd_h_ = ldh; }
        else { ldd_h_ = ld_; alloc((void**)&dH_, ldd_h_ * N_ * sizeof(ST)); }
        alloc((void**)&dV1_, ld_ * nc_ * sizeof(ST));
        alloc((void**)&dV2_, ld_ * nc_ * sizeof(ST));
        alloc((void**)&dD0_, N_ * sizeof(ST));
        alloc((void**)&dW_, N_ * nc_ * sizeof(T));
        w_cols_ = nc_;
        alloc((void**)&dA_, (a_elems ? a_elems : nc_ * nc_) * sizeof(T));
        alloc((void**)&dAs_, nc_ * nc_ * sizeof(ST));
    }
    ~ChaseHipSp() override
    {
        for (void* p : owned_) chase_hip_free(ctx_, p);
    }

    // ---- trivial getters ---------------------------------------------------------------------------------------
    std::size_t GetN() const override { return N_; }
    std::size_t GetNev() override { return nev_; }
    std::size_t GetNex() override { return nex_; }
    std::size_t GetLanczosIter() override { return lanczosIter_; }
    std::size_t GetNumLanczos() override { return numLanczos_; }
    std::size_t GetRitzvBlockSize() const override { return nc_; }
    R* GetRitzv() override { return ritzv_; }
    R* GetResid() override { return resid_.data(); }
    ConfigT& GetConfig() override { return config_; }
    int get_nprocs() override { return 1; }
    int get_rank() override { return 0; }
    bool isSym() override { return true; }
    bool isPseudoHerm() override { return false; }
    bool checkPseudoHermicityEasy() override { return false; }
    void Sort(R*, R*, R*) override {}
    void ApplyKconjugate(std::size_t) override {}
    void HEMM_H2(std::size_t, T, T, T, std::size_t, std::size_t = 0) override
    {
        throw std::logic_error("ChaseHipSp: HEMM_H2 belongs to the pseudo-Hermitian Impl");
    }
    void set_early_locked_residuals(std::vector<R> r) override { early_ = std::move(r); }
    std::size_t locked() const override { return locked_; }
    void* device_V1() override { flush_swaps(); return dV1_; }      // fp32: never to be read as fp64 (solver_capi.cpp guards)
    std::size_t local_rows() const override { return N_; }
    double filter_ms() const override { return filter_ms_; }
    std::size_t device_bytes() const override { return device_bytes_; }
    int last_qr_variant() const override { return last_qr_variant_; }
    std::size_t hemm_calls() const override { return 0; }
    std::size_t hemm_sp_calls() const override { return hemm_sp_calls_; }
    std::size_t hemm_sp_vecs() const override { return hemm_sp_vecs_; }
    std::size_t sp_filters() const override { return sp_filters_; }
    void set_device_rng(bool f) override
    {
        if (f) throw std::invalid_argument("device_rng: the single-precision solver draws its start vectors on the host");
    }
    void reset_counters() override { filter_ms_ = 0; hemm_sp_calls_ = 0; hemm_sp_vecs_ = 0; sp_filters_ = 0; }

    // randomized Hermiticity check: ||H v - H^H v|| small, both products accumulated into fp64; the threshold scales with 2^-24
    bool checkSymmetryEasy() override
    {
        CHASE_PHASE(ctx_, "checkSymmetryEasy");
        if (!h_resident_) upload_H();
        std::vector<ST> v(N_);
        std::mt19937 gen(1337);
        std::normal_distribution<> d;
        for (auto& x : v) x = rnd(d, gen);
        // transient: the fp32 vector and the two fp64 products (V2 keeps the start vectors LanczosDos copies back)
        void* blk = nullptr;
        int rc = chase_hip_malloc(ctx_, &blk, 2 * N_ * sizeof(T) + N_ * sizeof(ST));
        if (rc) throw HipStatusError(rc, "checkSymmetryEasy workspace");
        T* p = (T*)blk;
        ST* u = (ST*)(p + 2 * N_);
        std::vector<T> a(N_), b(N_);
        try {
            hip_ok(chase_hip_upload_matrix_sp(ctx_, CP, (int)N_, 1, v.data(), (long)N_, u, (long)N_), "upload");
            gemm32w('N', N_, 1, N_, dH_, ldd_h_, u, N_, p, N_);
            gemm32w('C', N_, 1, N_, dH_, ldd_h_, u, N_, p + N_, N_);
            hip_ok(chase_hip_download_matrix(ctx_, CP, (int)N_, 1, p, (long)N_, a.data(), (long)N_), "download");
            hip_ok(chase_hip_download_matrix(ctx_, CP, (int)N_, 1, p + N_, (long)N_, b.data(), (long)N_), "download");
        } catch (...) {
            chase_hip_free(ctx_, blk);
            throw;
        }
        chase_hip_free(ctx_, blk);
        double diff = 0, nrm = 0;
        for (std::size_t i = 0; i < N_; ++i) { diff += std::norm(a[i] - b[i]); nrm += std::norm(a[i]); }
        // the two products round differently by up to ~sqrt(N) 2^-24 of their size; an asymmetric entry shows at O(1) of it
        const double thr = 64.0 * std::sqrt((double)N_) * std::ldexp(1.0, -24);
        return std::sqrt(diff) <= thr * std::max(1.0, std::sqrt(nrm));
    }

    // complete the other triangle from `uplo` (reference: cpu::symOrHermMatrix): in HBM for a device matrix, else on the host copy
    void symOrHermMatrix(char uplo) override
    {
        if (h_on_device_) {
            hip_ok(chase_hip_complete_hermitian_sp(ctx_, CP, uplo, (int)N_, dH_, (long)ldd_h_), "complete_hermitian_sp");
            return;
        }
        const bool up = (uplo == 'U' || uplo == 'u');
        for (std::size_t j = 0; j < N_; ++j)
            for (std::size_t i = 0; i < j; ++i) {
                if (up) H_[j + i * ldh_] = conj_(H_[i + j * ldh_]);
                else    H_[i + j * ldh_] = conj_(H_[j + i * ldh_]);
            }
        h_resident_ = false;
    }

    // ---- solver life cycle -------------------------------------------------------------------------------------
    void Start() override { locked_ = 0; }

    // the same mt19937(1337) normals as ChaseHip (chase_cpu.hpp:296-327), rounded to fp32
    void initVecs(bool random) override
    {
        CHASE_PHASE(ctx_, "initVecs");
        if (random) {
            std::mt19937 gen(1337.0);
            std::normal_distribution<> d;
            for (std::size_t j = 0; j < nc_; ++j)
                for (std::size_t i = 0; i < N_; ++i) V1_[i + j * ldv_] = rnd(d, gen);
        }
        hip_ok(chase_hip_upload_matrix_sp(ctx_, CP, (int)N_, (int)nc_, V1_, (long)ldv_, dV1_, (long)ld_), "upload V");
        init_vecs_hook(random);
        hip_ok(chase_hip_lacpy_sp(ctx_, CP, (int)N_, (int)nc_, dV1_, (long)ld_, dV2_, (long)ld_), "lacpy_sp");
        reset_perm();
        upload_H();
    }

    // chase_cpu.hpp:329-349: re-randomise the given columns (offset by fixednev) of V1 from mt19937(4242) and mirror to V2
    void ReinitColumns(std::size_t fixednev, std::size_t const* col_indices, std::size_t n_indices) override
    {
        CHASE_PHASE(ctx_, "ReinitColumns");
        if (n_indices == 0) return;
        flush_swaps();
        std::mt19937 gen(4242);
        std::normal_distribution<> d;
        std::vector<ST> h(N_);
        for (std::size_t c = 0; c < n_indices; ++c) {
            const std::size_t j = fixednev + col_indices[c];
            if (j >= nc_) throw std::invalid_argument("ReinitColumns: column out of range");
            for (auto& x : h) x = rnd(d, gen);
            hip_ok(chase_hip_upload_matrix_sp(ctx_, CP, (int)N_, 1, h.data(), (long)N_, dV1_ + j * ld_, (long)ld_), "upload column");
            hip_ok(chase_hip_lacpy_sp(ctx_, CP, (int)N_, 1, dV1_ + j * ld_, (long)ld_, dV2_ + j * ld_, (long)ld_), "lacpy_sp");
        }
    }

    void End() override
    {
        CHASE_PHASE(ctx_, "End");
        flush_swaps();
        hip_ok(chase_hip_download_matrix_sp(ctx_, CP, (int)N_, (int)nc_, dV1_, (long)ld_, V1_, (long)ldv_), "download V");
    }

    // ---- filter --------------------------------------------------------------------------------------------------
    void FilterPhaseStart() override
    {
        roctx_push("chase:Filter");
        flush_swaps();
        chase_hip_ctx_set_phase(ctx_, 1);
        hip_ok(chase_hip_timer_start(ctx_), "timer");
        ++sp_filters_;
    }
    void FilterPhaseEnd() override
    {
        float ms = 0;
        hip_ok(chase_hip_timer_stop(ctx_, &ms), "timer");
        chase_hip_ctx_set_phase(ctx_, 0);
        filter_ms_ += ms;
        roctx_pop(ctx_);
    }

    // H_ii = fl32(d0_i + s), s the accumulated shift; the diagonal is saved whenever a shift starts from s == 0 (so a matrix
    // the caller changed between solves is picked up), and the unshift ends the bracket: s = 0, the saved bits are back
    void Shift(T c, bool isunshift = false) override
    {
        if (!h_resident_) upload_H();
        if (shift_ == 0.0) {
            // the N diagonal entries are the 1 x N matrix of leading dimension ld + 1
            hip_ok(chase_hip_lacpy_sp(ctx_, CP, 1, (int)N_, dH_, (long)ldd_h_ + 1, dD0_, 1), "save diagonal");
        }
        shift_ = isunshift ? 0.0 : shift_ + (double)std::real(c);
        hip_ok(chase_hip_shift_diag_sp(ctx_, CP, (int)N_, dH_, (long)ldd_h_, dD0_, shift_), "shift_diag_sp");
    }

    // V2[:, c0:c0+ncols] = alpha * H * V1[:, c0:...] + beta * V2[:, ...], c0 = locked + offset_left; then V1 <-> V2
    void HEMM(std::size_t block, T alpha, T beta, std::size_t offset_left, std::size_t offset_right = 0) override
    {
        flush_swaps();
        const std::size_t ncols = (offset_right < block) ? block - offset_right : 0;
        if (ncols != 0) {
            const std::size_t c0 = locked_ + offset_left;
            if (c0 + ncols > nevex_) throw std::invalid_argument("HEMM: columns beyond the block");
            gemm32(N_, ncols, N_, alpha, dH_, ldd_h_, dV1_ + c0 * ld_, ld_, beta, dV2_ + c0 * ld_, ld_);
            ++hemm_sp_calls_;
            hemm_sp_vecs_ += ncols;
        }
        std::swap(dV1_, dV2_);
    }

    // ---- QR in fp64 on the widened block (QR_DOUBLE_PRECISION) -----------------------------------------------------------
    void QR(std::size_t, R cond) override
    {
        CHASE_PHASE(ctx_, "QR");
        flush_swaps();
        hip_ok(chase_hip_lacpy_sp(ctx_, CP, (int)N_, (int)locked_, dV1_, (long)ld_, dV2_, (long)ld_), "lacpy_sp");
        qr_block(cond);
        hip_ok(chase_hip_lacpy_sp(ctx_, CP, (int)N_, (int)locked_, dV2_, (long)ld_, dV1_, (long)ld_), "lacpy_sp");
    }

    // ---- Rayleigh-Ritz ---------------------------------------------------------------------------------------------------
    void RR(R* ritzv, std::size_t block) override
    {
        CHASE_PHASE(ctx_, "RR");
        flush_swaps();
        if (locked_ + block > nevex_) throw std::invalid_argument("RR: columns beyond the block");
        ST* Q = dV1_ + locked_ * ld_;
        ST* W = dV2_ + locked_ * ld_;
        gemm32(N_, block, N_, T(1), dH_, ldd_h_, Q, ld_, T(0), W, ld_);                     // W = H Q (H = H^H)
        gemm32w('C', block, block, N_, Q, ld_, W, ld_, dA_, block);                         // A = Q^H W in fp64
        hip_ok(chase_hip_heevd(ctx_, CP, (int)block, dA_, (long)block, ritzv), "heevd");
        hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)block, (int)block, dA_, (long)block, dAs_, (long)block), "convert_d2s");
        gemm32(N_, block, block, T(1), Q, ld_, dAs_, block, T(0), W, ld_);                  // W = Q A
        std::swap(dV1_, dV2_);
    }

    // ---- residuals ---------------------------------------------------------------------------------------------------------
    void Resd(R* ritzv, R* resd, std::size_t) override
    {
        CHASE_PHASE(ctx_, "Resd");
        flush_swaps();
        const std::size_t sub = nevex_ - locked_;
        ST* V = dV1_ + locked_ * ld_;
        ST* W = dV2_ + locked_ * ld_;
        gemm32(N_, sub, N_, T(1), dH_, ldd_h_, V, ld_, T(0), W, ld_);
        hip_ok(chase_hip_resid_norms_sp(ctx_, CP, (int)N_, (int)sub, W, (long)ld_, V, (long)ld_, ritzv, resd), "resid_norms_sp");
        if (resd != resid_.data() + locked_) std::memcpy(resid_.data() + locked_, resd, sub * sizeof(R));
    }

    void recompute_residuals(std::size_t ncols, const double* lambda, double* out) override
    {
        CHASE_PHASE(ctx_, "recompute_residuals");
        if (ncols > nc_) throw std::invalid_argument("recompute_residuals: more columns than the Impl holds");
        flush_swaps();
        if (!h_resident_) upload_H();
        gemm32(N_, ncols, N_, T(1), dH_, ldd_h_, dV1_, ld_, T(0), dV2_, ld_);             // dV2_ is scratch from here on
        hip_ok(chase_hip_resid_norms_sp(ctx_, CP, (int)N_, (int)ncols, dV2_, (long)ld_, dV1_, (long)ld_, lambda, out), "resid_norms_sp");
    }

    void Swap(std::size_t i, std::size_t j) override
    {
        if (i == j) return;
        if (i >= nc_ || j >= nc_) throw std::invalid_argument("Swap: column out of range");
        std::swap(perm_[i], perm_[j]);
        perm_dirty_ = true;
    }
    void Lock(std::size_t new_converged) override
    {
        if (locked_ + new_converged > nevex_) throw std::invalid_argument("Lock: more columns than the block holds");
        locked_ += new_converged;
    }

    // ---- Lanczos (cpu/lanczos.hpp:46-209, :216-300) -------------------------------------------------------------------
    void Lanczos(std::size_t m, R* upperb) override
    {
        CHASE_PHASE(ctx_, "Lanczos");
        lanczosIter_ = m; numLanczos_ = 1;
        std::vector<R> theta(m);
        lanczos_core(m, 1, false, upperb, theta.data(), nullptr, nullptr);
    }
    void Lanczos(std::size_t M, std::size_t numvec, R* upperb, R* ritzv, R* Tau, R* ritzV) override
    {
        CHASE_PHASE(ctx_, "Lanczos");
        lanczosIter_ = M; numLanczos_ = numvec;
        lanczos_core(M, numvec, true, upperb, ritzv, Tau, ritzV);
    }
    // V1[:, :idx] <- V1[:, :m] * ritzVc[:, :idx] accumulated into fp64 and rounded into V1 (chase_cpu.hpp:368-382)
    void LanczosDos(std::size_t idx, std::size_t m, T* ritzVc) override
    {
        CHASE_PHASE(ctx_, "LanczosDos");
        flush_swaps();
        if (m > nc_ || idx > m) throw std::invalid_argument("LanczosDos: more Lanczos vectors than the block holds");
        hip_ok(chase_hip_upload_matrix(ctx_, CP, (int)m, (int)idx, ritzVc, (long)m, dA_, (long)m), "upload ritzV");
        hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)m, (int)idx, dA_, (long)m, dAs_, (long)m), "convert_d2s");
        gemm32w('N', N_, idx, m, dV1_, ld_, dAs_, m, dW_, N_);
        hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)N_, (int)idx, dW_, (long)N_, dV1_, (long)ld_), "convert_d2s");
        // the reference copies m columns of its work block back, so columns idx .. m-1 become those of V2 (the start vectors)
        hip_ok(chase_hip_lacpy_sp(ctx_, CP, (int)N_, (int)(m - idx), dV2_ + idx * ld_, (long)ld_, dV1_ + idx * ld_, (long)ld_), "lacpy_sp");
    }

    // the current block widened to fp64 on the host (N x all columns of the block, ld): what chase_hip_solver_peek_v returns
    void peek_widened(T* host, std::size_t ld)
    {
        flush_swaps();
        if (ld < N_) throw std::invalid_argument("peek_v: leading dimension smaller than N");
        std::vector<ST> h(N_ * nc_);
        hip_ok(chase_hip_download_matrix_sp(ctx_, CP, (int)N_, (int)nc_, dV1_, (long)ld_, h.data(), (long)N_), "download V");
        for (std::size_t j = 0; j < nc_; ++j)
            for (std::size_t i = 0; i < N_; ++i) host[i + j * ld] = T(h[i + j * N_]);
    }

protected:
    // after the start block is uploaded, before it is mirrored to V2 (the pseudo-Hermitian Impl damps the lower rows)
    virtual void init_vecs_hook(bool) {}
    // after all columns of V1 are widened into dW_, before they are factorised (the pseudo-Hermitian Impl flips the locked ones)
    virtual void qr_widened_hook() {}

    // QR_DOUBLE_PRECISION on all nc_ columns of V1: widened into the fp64 scratch, CholQR1 / CholQR2 / shifted CholQR2 or Householder
    // there with the single-precision thresholds, rounded back
    void qr_block(R cond)
    {
        hip_ok(chase_hip_convert_s2d(ctx_, CP, (int)N_, (int)nc_, dV1_, (long)ld_, dW_, (long)N_), "convert_s2d");
        qr_widened_hook();
        int disable = config_.DoCholQR() ? 0 : 1;
        if (const char* s = std::getenv("CHASE_DISABLE_CHOLQR")) disable = std::atoi(s);
        R thld_hi = 1e4, thld_lo = 1e1;                 // chase_gpu.hpp:808-809, float
        if (const char* s = std::getenv("CHASE_CHOLQR1_THLD")) thld_lo = std::atof(s);
        last_qr_variant_ = 0;
        if (disable == 1 && cond != (R)1.0) {
            hip_ok(chase_hip_houseqr(ctx_, CP, (int)N_, (int)nc_, dW_, (long)N_), "houseqr");
        } else {
            const int variant = (cond > thld_hi) ? 3 : (cond < thld_lo ? 1 : 2);
            last_qr_variant_ = variant;
            const int info = chase_hip_cholqr(ctx_, CP, (int)N_, (int)nc_, dW_, (long)N_, dA_, (long)nc_, variant, (long)N_);
            hip_ok(info, "cholqr");
            if (info != 0) {
                last_qr_variant_ = 0;
                // a failed factorisation leaves the block as it was (cholqr1.hpp:41-68): Householder on the same widened columns
                hip_ok(chase_hip_convert_s2d(ctx_, CP, (int)N_, (int)nc_, dV1_, (long)ld_, dW_, (long)N_), "convert_s2d");
                qr_widened_hook();
                hip_ok(chase_hip_houseqr(ctx_, CP, (int)N_, (int)nc_, dW_, (long)N_), "houseqr");
            }
        }
        hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)N_, (int)nc_, dW_, (long)N_, dV1_, (long)ld_), "convert_d2s");
    }

    static ST rnd(std::normal_distribution<>& d, std::mt19937& g)
    {
        if constexpr (is_cplx<T>::value) { const double re = d(g); const double im = d(g); return ST((float)re, (float)im); }
        else return ST(d(g));
    }
    static ST conj_(ST x) { if constexpr (is_cplx<T>::value) return std::conj(x); else return x; }
    // leading dimension of the device blocks: every column starts on a 16-byte boundary
    static std::size_t shadow_ld(std::size_t n) { return (n + 3) & ~(std::size_t)3; }

    void alloc(void** p, std::size_t bytes)
    {
        int rc = chase_hip_malloc(ctx_, p, bytes);
        if (rc) throw HipStatusError(rc, "chase_hip_malloc");
        owned_.push_back(*p);
        device_bytes_ += bytes;
    }
    void upload_H()
    {
        if (!h_on_device_)
            hip_ok(chase_hip_upload_matrix_sp(ctx_, CP, (int)N_, (int)N_, H_, (long)ldh_, dH_, (long)ldd_h_), "upload H");
        h_resident_ = true;
        shift_ = 0.0;
    }
    void gemm32(std::size_t m, std::size_t n, std::size_t k, T alpha, const ST* A, std::size_t lda, const ST* B, std::size_t ldb,
                T beta, ST* C, std::size_t ldc)
    {
        int rc;
        if constexpr (is_cplx<T>::value) {
            const float a[2] = {(float)alpha.real(), (float)alpha.imag()}, b[2] = {(float)beta.real(), (float)beta.imag()};
            rc = chase_hip_gemm_c(ctx_, 'N', (int)m, (int)n, (int)k, a, A, (long)lda, B, (long)ldb, b, C, (long)ldc);
        } else {
            rc = chase_hip_gemm_s(ctx_, 'N', (int)m, (int)n, (int)k, (float)alpha, A, (long)lda, B, (long)ldb, (float)beta, C, (long)ldc);
        }
        hip_ok(rc, "gemm32");
    }
    // C64 = op(A32) B32: fp32 operands on the f32 matrix cores, fp64 result
    void gemm32w(char op, std::size_t m, std::size_t n, std::size_t k, const ST* A, std::size_t lda, const ST* B, std::size_t ldb, T* C,
                 std::size_t ldc)
    {
        int rc;
        if constexpr (is_cplx<T>::value) {
            const double one[2] = {1.0, 0.0}, zero[2] = {0.0, 0.0};
            rc = chase_hip_gemm_cz(ctx_, op, (int)m, (int)n, (int)k, one, A, (long)lda, B, (long)ldb, zero, C, (long)ldc);
        } else {
            rc = chase_hip_gemm_sd(ctx_, op, (int)m, (int)n, (int)k, 1.0, A, (long)lda, B, (long)ldb, 0.0, C, (long)ldc);
        }
        hip_ok(rc, "gemm32w");
    }
    void reset_perm()
    {
        for (std::size_t i = 0; i < nc_; ++i) perm_[i] = (int)i;
        perm_dirty_ = false;
    }
    // apply the deferred swaps: V1'[:, j] = V1[:, perm[j]] through V2 (free whenever swaps are pending)
    void flush_swaps()
    {
        if (!perm_dirty_) return;
        std::vector<int> src, dst;
        for (std::size_t j = 0; j < nc_; ++j)
            if (perm_[j] != (int)j) { src.push_back(perm_[j]); dst.push_back((int)j); }
        if (!src.empty())
            hip_ok(chase_hip_permute_cols_sp(ctx_, CP, (int)N_, dV1_, (long)ld_, dV2_, (long)ld_, src.data(), dst.data(),
                                             (int)src.size()), "permute_cols_sp");
        reset_perm();
    }

    // the fp64 scratch holds the three blocks of nv Lanczos vectors (grown when 3 nv > nev + nex); the scalars and the fp32 copy
    // of the current block that the product reads are a transient allocation of O(N nv)
    void lanczos_core(std::size_t M, std::size_t nv, bool store, R* upperb, R* theta, R* Tau, R* ritzV)
    {
        flush_swaps();
        if (!h_resident_) upload_H();
        if (nv == 0 || nv > nevex_ || M == 0 || (store && M > nevex_))
            throw std::invalid_argument("Lanczos: more vectors or steps than the block holds");
        constexpr int E = CP ? 2 : 1;
        if (3 * nv > w_cols_) {
            alloc((void**)&dW_, N_ * 3 * nv * sizeof(T));       // (the smaller scratch stays owned until the Impl goes)
            w_cols_ = 3 * nv;
        }
        T *v0 = dW_, *v1 = v0 + N_ * nv, *v2 = v1 + N_ * nv;
        void* blk = nullptr;
        const std::size_t s_bytes = ld_ * nv * sizeof(ST);
        const std::size_t sc_bytes = (M * nv * E + M * nv + nv) * sizeof(double);
        int rc = chase_hip_malloc(ctx_, &blk, s_bytes + sc_bytes);
        if (rc) throw HipStatusError(rc, "lanczos workspace");
        ST* s1 = (ST*)blk;
        double* d_alpha = (double*)((char*)blk + s_bytes);
        double* d_beta = d_alpha + M * nv * E;
        double* d_nrm0 = d_beta + M * nv;
        const int n = (int)N_, nvi = (int)nv;
        try {
            hip_ok(chase_hip_memset(ctx_, blk, 0, s_bytes + sc_bytes), "memset");
            hip_ok(chase_hip_memset(ctx_, dW_, 0, N_ * 3 * nv * sizeof(T)), "memset");
            hip_ok(chase_hip_convert_s2d(ctx_, CP, n, nvi, dV1_, (long)ld_, v1, (long)N_), "convert_s2d");
            hip_ok(chase_hip_col_nrm2(ctx_, CP, n, nvi, v1, (long)N_, d_nrm0), "nrm2");
            hip_ok(chase_hip_col_scal(ctx_, CP, n, nvi, d_nrm0, 1, v1, (long)N_), "scal");
            for (std::size_t k = 0; k < M; ++k) {
                hip_ok(chase_hip_convert_d2s(ctx_, CP, n, nvi, v1, (long)N_, s1, (long)ld_), "convert_d2s");
                // the reference writes every run's k-th vector into column k (last run wins), cpu/lanczos.hpp:85-88
                if (store)
                    hip_ok(chase_hip_lacpy_sp(ctx_, CP, n, 1, s1 + (nv - 1) * ld_, (long)ld_, dV1_ + k * ld_, (long)ld_), "lacpy_sp");
                gemm32w('N', N_, nv, N_, dH_, ldd_h_, s1, ld_, v2, N_);                   // H = H^H
                double* ak = d_alpha + k * nv * E;
                hip_ok(chase_hip_col_dot(ctx_, CP, n, nvi, v1, (long)N_, v2, (long)N_, ak), "dot");
                hip_ok(chase_hip_col_axpy(ctx_, CP, n, nvi, ak, 0, 1, -1.0, v1, (long)N_, v2, (long)N_), "axpy");
                if (k > 0)
                    hip_ok(chase_hip_col_axpy(ctx_, CP, n, nvi, d_beta + (k - 1) * nv, 1, 1, -1.0, v0, (long)N_, v2, (long)N_), "axpy");
                hip_ok(chase_hip_col_nrm2(ctx_, CP, n, nvi, v2, (long)N_, d_beta + k * nv), "nrm2");
                if (k == M - 1) break;
                hip_ok(chase_hip_col_scal(ctx_, CP, n, nvi, d_beta + k * nv, 1, v2, (long)N_), "scal");
                T* t = v0; v0 = v1; v1 = v2; v2 = t;
            }
            if (store) hip_ok(chase_hip_convert_d2s(ctx_, CP, n, nvi, v1, (long)N_, dV1_, (long)ld_), "convert_d2s");
            std::vector<double> h_alpha(M * nv * E), h_beta(M * nv);
            hip_ok(chase_hip_memcpy_d2h(ctx_, h_alpha.data(), d_alpha, h_alpha.size() * sizeof(double)), "d2h");
            hip_ok(chase_hip_memcpy_d2h(ctx_, h_beta.data(), d_beta, h_beta.size() * sizeof(double)), "d2h");
            chase_hip_free(ctx_, blk);
            blk = nullptr;

            std::vector<double> d(M), e(M), w(M), Z(M * M);
            R ub = 0;
            for (std::size_t i = 0; i < nv; ++i) {
                for (std::size_t k = 0; k < M; ++k) {
                    d[k] = h_alpha[(k * nv + i) * E];
                    e[k] = (k + 1 < M) ? h_beta[k * nv + i] : 0.0;
                }
                hip_ok(chase_hip_stemr_host((int)M, d.data(), e.data(), w.data(), Z.data(), (int)M), "stemr");
                for (std::size_t k = 0; k < M; ++k) {
                    theta[k + i * M] = w[k];
                    if (Tau) Tau[k + i * M] = std::abs(Z[k * M]) * std::abs(Z[k * M]);
                }
                if (ritzV) std::memcpy(ritzV, Z.data(), M * M * sizeof(double));   // last run wins, like the reference
                const R cand = std::max(std::abs(w[0]), std::abs(w[M - 1])) + std::abs(h_beta[(M - 1) * nv + i]);
                ub = (i == 0) ? cand : std::max(ub, cand);
            }
            *upperb = ub;
        } catch (...) {
            if (blk) chase_hip_free(ctx_, blk);
            throw;
        }
    }

    chase_hip_ctx* ctx_;
    std::size_t N_, nev_, nex_, nevex_, nc_;          // nc_: columns of the vector blocks (nevex_ here, 2 nevex_ pseudo-Hermitian)
    ST* H_; std::size_t ldh_;
    ST* V1_; std::size_t ldv_;
    R* ritzv_;
    bool h_on_device_, h_resident_ = false;
    ConfigT config_;
    std::vector<R> resid_, early_;
    std::vector<int> perm_;
    bool perm_dirty_ = false;
    std::size_t locked_ = 0, lanczosIter_ = 0, numLanczos_ = 0;
    ST *dH_ = nullptr, *dV1_ = nullptr, *dV2_ = nullptr, *dD0_ = nullptr, *dAs_ = nullptr;   // fp32: H, the blocks, saved diagonal, A
    T *dW_ = nullptr, *dA_ = nullptr;                                                       // fp64: N x w_cols_ scratch, projected matrix
    std::size_t ld_ = 0, ldd_h_ = 0, w_cols_ = 0;
    double shift_ = 0.0;                   // accumulated shift of the resident H
    std::vector<void*> owned_;
    std::size_t device_bytes_ = 0;
    double filter_ms_ = 0;
    std::size_t hemm_sp_calls_ = 0, hemm_sp_vecs_ = 0, sp_filters_ = 0;
    int last_qr_variant_ = 0;
};

} // namespace chase_amd
