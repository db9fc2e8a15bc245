// impl_extras.hpp — what the C entry points, the bench and the tape (tape.hpp) need from an Impl beyond the ChaseBase surface.
// No HIP, no C ABI: includable by host-only test programs.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace chase_amd {

// what the C entry points and the bench need beyond the ChaseBase surface, common to both Impls
struct HipImplExtras {
    virtual ~HipImplExtras() = default;
    virtual std::size_t locked() const = 0;
    virtual int last_qr_variant() const = 0;     // 0 = Householder, 1/2/3 = CholQR1 / CholQR2 / shifted CholQR2
    virtual double filter_ms() const = 0;        // HIP-event time between FilterPhaseStart/End, accumulated
    virtual std::size_t hemm_calls() const = 0;
    virtual std::size_t hemm_reused_vecs() const { return 0; }   // filter columns served from RR's cached H V (no GEMM)
    virtual std::size_t resd_rechecked() const { return 0; }     // residuals re-taken from a fresh four-product H v (on the tolerance)
    // mixed-precision filter (the Hermitian Impls, single GPU and grid): false = this Impl has no fp32 path and `on` was not taken
    virtual bool set_mixed_precision(bool on) { return !on; }
    virtual bool mixed_precision() const { return false; }
    virtual std::size_t hemm_sp_calls() const { return 0; }      // fp32 filter products
    virtual std::size_t hemm_sp_vecs() const { return 0; }       // columns filtered in fp32
    virtual std::size_t sp_filters() const { return 0; }         // filter calls that ran in fp32
    // which product a filter call in single precision uses: 0 = fp32 MFMA (default), 1 = bf16x3 (split operands on the bf16
    // matrix cores); no effect while mixed_precision is off.  false = this Impl has no fp32 path and v != 0 was not taken
    virtual bool set_sp_product(int v) { return v == 0; }
    virtual int sp_product() const { return 0; }
    virtual std::size_t hemm_sp_split_calls() const { return 0; }   // fp32 filter products that ran as bf16x3
    // sp_prepack: a single-precision filter call that runs bf16x3 (sp_product = 1) takes H split and tiled once
    // (chase_hip_gemm_*_bf16x3p) - the same bits; inert otherwise.  false = this Impl does not have it and v != 0 was not taken
    virtual bool set_sp_prepack(int v) { return v == 0; }
    virtual int sp_prepack() const { return 0; }
    virtual std::size_t hemm_sp_packed_calls() const { return 0; }  // the hemm_sp_split_calls that ran on the packed H
    virtual std::size_t sp_pack_full() const { return 0; }          // whole-matrix packs of H
    virtual std::size_t sp_pack_diag() const { return 0; }          // diagonal refreshes of the pack
    // h2_mixed_precision (the single-GPU pseudo-Hermitian Impl): an H^2 filter call that starts while the smallest residual of the
    // unlocked wanted pairs is above 1e-3 runs its products in fp32.  A key of its own: mixed_precision stays the Hermitian
    // solvers'.  false = this Impl has no fp32 H^2 filter and `on` was not taken
    virtual bool set_h2_mixed_precision(bool on) { return !on; }
    virtual bool h2_mixed_precision() const { return false; }
    virtual std::size_t sp_h_converts() const { return 0; }         // whole-matrix fp64 -> fp32 conversions of H (that Impl)
    virtual std::size_t device_bytes() const { return 0; }          // sum of the Impl's own device allocations (single-GPU Impls)
    virtual void set_device_rng(bool) = 0;
    virtual void reset_counters() = 0;
    virtual void* device_V1() = 0;               // current (local) vector block, pending swaps applied
    virtual std::size_t local_rows() const = 0;
    // out[j] = || H v_j - lambda_j v_j ||_2 for the first ncols vectors the Impl holds, from a FRESH four-product H V
    // (never from products a previous step left behind): what the reference's solve tests recompute after a solve
    // (tests/chase_serial_solve.cpp:144-148,195-199, tests/chase_distributed_solve.cpp:209-284)
    virtual void recompute_residuals(std::size_t ncols, const double* lambda, double* out) = 0;
    // k >= 0: the next Resd re-takes the residuals of its first k columns from a fresh four-product H v whatever their
    // values (single-rank replay: as many as the recorded solve re-took on the tolerance, tape.hpp); -1: by value (default)
    virtual void set_forced_recheck(long) {}
    // v >= 0: the next QR takes variant v (0 Householder, 1/2/3 CholQR1 / CholQR2 / shifted CholQR2) whatever its data say -
    // a Cholesky factorisation that fails on the replayed rank's numbers is retried on a shifted Gram matrix instead of
    // falling back to Householder (single-rank replay follows the recording's QR variants, tape.hpp); -1: by data (default)
    virtual void set_forced_qr(int) {}
    virtual std::size_t forced_qr_retries() const { return 0; }
    // single-rank replay of the pseudo-Hermitian solve: the lone rank's projected matrices are partial sums - when Q^H S H Q does
    // not factorise, Rayleigh-Ritz runs the same operators on the identity instead of throwing; a Lanczos tridiagonal the host
    // eigensolver rejects yields zeros (the driver reads the tape's numbers either way)
    virtual void set_replay_tolerant(bool) {}
    virtual std::size_t replay_tolerated() const { return 0; }
    // phase marker of the profiler ranges (CHASE_HIP_ROCTX=1, roctx.hpp): nothing to implement
};

// CHASE_HIP_MIXED_PRECISION=1 reaches Impls without an fp32 filter through the environment of a whole application: said once
inline void mixed_precision_env_ignored(const char* impl)
{
    static std::atomic<bool> said{false};          // (ranks of a grid may be threads of one process)
    const char* e = std::getenv("CHASE_HIP_MIXED_PRECISION");
    if (!e || std::atoi(e) == 0 || said.exchange(true)) return;
    std::fprintf(stderr, "chase_hip: CHASE_HIP_MIXED_PRECISION is ignored by %s (Hermitian solvers only)\n", impl);
}

// CHASE_HIP_SP_PRODUCT=bf16x3|f32: the construction-time default of sp_product (anything else: f32)
inline int sp_product_env()
{
    const char* e = std::getenv("CHASE_HIP_SP_PRODUCT");
    return e && std::strcmp(e, "bf16x3") == 0 ? 1 : 0;
}
inline void sp_product_env_ignored(const char* impl)
{
    static std::atomic<bool> said{false};
    if (sp_product_env() == 0 || said.exchange(true)) return;
    std::fprintf(stderr, "chase_hip: CHASE_HIP_SP_PRODUCT is ignored by %s (Hermitian solvers only)\n", impl);
}

// CHASE_HIP_SP_PREPACK=1: the construction-time default of sp_prepack
inline int sp_prepack_env()
{
    const char* e = std::getenv("CHASE_HIP_SP_PREPACK");
    return e && std::atoi(e) != 0 ? 1 : 0;
}
inline void sp_prepack_env_ignored(const char* impl)
{
    static std::atomic<bool> said{false};
    if (sp_prepack_env() == 0 || said.exchange(true)) return;
    std::fprintf(stderr, "chase_hip: CHASE_HIP_SP_PREPACK is ignored by %s (single-GPU Hermitian solver only)\n", impl);
}

// CHASE_HIP_H2_MIXED_PRECISION=1: the construction-time default of h2_mixed_precision
inline int h2_mixed_precision_env()
{
    const char* e = std::getenv("CHASE_HIP_H2_MIXED_PRECISION");
    return e && std::atoi(e) != 0 ? 1 : 0;
}

} // namespace chase_amd
