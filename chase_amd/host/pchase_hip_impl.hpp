// pchase_hip_impl.hpp — pChaseHip<T, BaseT>: multi-GPU implementation of the ChaseBase<T> operator surface on a 2D
// process grid, one process per MI355X, collectives over RCCL/xGMI.
//
// Semantics follow the reference's distributed Impls virtual by virtual
//   Impl/pchase_cpu/pchase_cpu.hpp:92-1129 (pChASECPU)  and  Impl/pchase_gpu/pchase_gpu.hpp:119-1804 (pChASEGPU<NCCL>)
// and their kernels
//   HEMM           linalg/internal/mpi/hemm.hpp:46-230        (column-type <-> row-type, beta on grid row/col 0, all-reduce)
//   CholQR         linalg/internal/mpi/cholqr.hpp:51-397      (Gram all-reduce over the column communicator)
//   Rayleigh-Ritz  linalg/internal/mpi/rayleighRitz.hpp:103-186
//   residuals      linalg/internal/mpi/residuals.hpp:61-107
//   Lanczos        linalg/internal/mpi/lanczos.hpp:153-370
//   redistribution linalg/distMatrix/distMultiVector.hpp:2444-2720 (one packed broadcast per source rank here,
//                  instead of one per contiguous run: 2 instead of 1024 for block-cyclic nb = 64 at N = 65536)
// Data distribution: H block-cyclic (mb x nb; a block layout is mb = block length) over nprow x npcol;
// "column-type" multivectors V1/V2 are split like H's rows over the grid rows and replicated over grid columns,
// "row-type" W1/W2 are split like H's columns over the grid columns and replicated over grid rows.
//
// MI355X-first differences from the reference (results equal up to rounding):
//   * the filter HEMM is panel-pipelined: the all-reduce of column panel p runs on the communication stream while the
//     MFMA GEMM of panel p+1 runs on the compute stream, and the next filter step's GEMM on panel p waits only for
//     panel p's all-reduce (the reference left this as commented-out code, linalg/internal/nccl/hemm.hpp:97-288);
//   * host control flow (potrf info, Ritz values, residuals) is made identical on all ranks by tiny agreement
//     collectives instead of relying on bitwise-identical replicas;
//   * Swap() is deferred into one column permutation, Lanczos scalars stay on the device;
//   * mixed-precision filter (reference: pchase_gpu.hpp:785-901, CHASE_ENABLE_MIXED_PRECISION at build time) behind the run-time
//     switch of ChaseHip, default off: set_mixed_precision / CHASE_HIP_MIXED_PRECISION=1.  A filter call that starts while the
//     smallest residual of the unlocked wanted pairs is above 1e-3 runs its local products on fp32 operands (a shadow of H_loc,
//     the input panel converted on the way) on the f32-input matrix cores, but every rank's partial product is WRITTEN AND SUMMED
//     IN FP64: the vector blocks, the all-reduces, the transports and the panel pipeline are those of the fp64 path, nothing is
//     converted back, locked columns are never touched.  fp32 collectives (half the bytes) are a later step;
//   * the Householder fallback pivots in the stacked row order and fuses each column's three scalar all-reduces into one.
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <stdexcept>
#include <vector>
#include "../../include/chase_hip.h"
#include "../../include/chase_hip_grid.h"
#include "chase_hip_impl.hpp"
#include "interface.hpp"
#include "output_override.hpp"
#include "panel_pipeline.hpp"
#include "roctx.hpp"

namespace chase_amd {

template <class T, class BaseT = ChaseBase<T>, class ConfigT = ChaseConfig<T>>
class pChaseHip : public WithOutput<BaseT>, public HipImplExtras {
public:
    using R = Base<T>;
    static constexpr int CP = is_cplx<T>::value ? 1 : 0;
    static constexpr int E = CP ? 2 : 1;
    using ST = std::conditional_t<is_cplx<T>::value, std::complex<float>, float>;      // element of the fp32 shadows

    struct Dim {                                      // 1D block-cyclic distribution of N indices over p ranks
        long N = 0, nb = 1; int p = 1, q = 0; long nloc = 0;
        int owner(long g) const { return chase_hip_owner(g, nb, p); }
        long local(long g) const { return chase_hip_local_index(g, nb, p); }
        long global(long l, int iq) const { return chase_hip_global_index(l, nb, iq, p); }
        long count(int iq) const { return chase_hip_numroc(N, nb, iq, p); }
    };

    // H_loc: DEVICE pointer to this rank's m_loc x n_loc block (ldh >= m_loc).  mb = nb = 0 selects the block layout.
    // ncols: number of columns of the vector blocks (nev+nex; the pseudo-Hermitian Impl derives with 2*(nev+nex))
    pChaseHip(chase_hip_ctx* ctx, chase_hip_grid* grid, std::size_t N, std::size_t nev, std::size_t nex, std::size_t mb,
              std::size_t nb, T* H_loc, std::size_t ldh, R* ritzv, std::size_t ncols = 0)
        : ctx_(ctx), grid_(grid), N_(N), nev_(nev), nex_(nex), nevex_(nev + nex), nc_(ncols ? ncols : nev + nex),
          dH_(H_loc), ldh_(ldh), ritzv_(ritzv), config_(N, nev, nex), resid_(ncols ? ncols : nev + nex, 0),
          perm_(ncols ? ncols : nev + nex)
    {
        if (!ctx || !grid || !H_loc || !ritzv) throw std::invalid_argument("pChaseHip: null argument");
        if (N == 0 || nevex_ == 0 || nc_ > N) throw std::invalid_argument("pChaseHip: need 0 < nev+nex <= N");
        if (const char* e = std::getenv("CHASE_HIP_MIXED_PRECISION")) mixed_ = std::atoi(e) != 0;   // (the pseudo Impl clears it)
        sp_split_ = sp_product_env() != 0;                                                         // (and this)
        sp_prepack_env_ignored("the grid solvers");            // (op C and the fp64 epilogue from a packed block: not built)
        hip_ok(chase_hip_grid_info(grid, &nprow_, &npcol_, &myrow_, &mycol_), "grid_info");
        Rr_.N = Cc_.N = (long)N;
        Rr_.p = nprow_; Rr_.q = myrow_; Cc_.p = npcol_; Cc_.q = mycol_;
        Rr_.nb = mb ? (long)mb : chase_hip_block_len((long)N, nprow_);
        Cc_.nb = nb ? (long)nb : chase_hip_block_len((long)N, npcol_);
        Rr_.nloc = Rr_.count(myrow_);
        Cc_.nloc = Cc_.count(mycol_);
        m_ = (std::size_t)Rr_.nloc; n_ = (std::size_t)Cc_.nloc;
        if (ldh < m_) throw std::invalid_argument("pChaseHip: ldh smaller than the local row count");
        // a rank may own NO rows or columns: the reference's block rule (distMatrix.hpp:1992-2052) gives the last rank of a
        // dimension N - (p - 1) len of them, which is 0 for N = 9 on 4 grid rows (3, 3, 3, 0) - such a rank takes part in
        // every collective with empty blocks (all products, copies and reductions below accept zero rows)
        for (std::size_t i = 0; i < nc_; ++i) perm_[i] = (int)i;
        alloc((void**)&dV1_, m_ * nc_ * sizeof(T));
        alloc((void**)&dV2_, m_ * nc_ * sizeof(T));
        alloc((void**)&dVt_, m_ * nc_ * sizeof(T));
        alloc((void**)&dW1_, n_ * nc_ * sizeof(T));
        alloc((void**)&dW2_, n_ * nc_ * sizeof(T));
        alloc((void**)&dA_, 3 * nc_ * nc_ * sizeof(T));
        pack_elems_ = nc_ * nc_ + 64 * nc_ + 64;                    // packed Gram triangle / agreement scratch
        alloc((void**)&dPack_, pack_elems_ * sizeof(T));
        // staging must hold the largest block of ANY rank (rank 0 of a dimension owns the most rows)
        // staging of the column <-> row redistribution: the pieces of ALL source ranks side by side (they add up to the rows
        // of the destination block), so that the broadcasts can be in flight together
        stage_rows_ = (std::size_t)std::max(std::max(Rr_.count(0), Cc_.count(0)), (long)std::max(m_, n_));
        alloc((void**)&dStage_, stage_rows_ * nc_ * sizeof(T));
        dHbac_ = dH_; ldhbac_ = ldh_;
        // column panel of the pipelined HEMM: a panel's GEMM should fill the chip once with whole output tiles
        // (128-row tiles x 64 / 128 columns, two workgroups on each of the 256 CUs) in both directions; the panel grid is
        // fixed for the object's life time (the per-panel events are indexed by it)
        {
            const std::size_t bn = CP ? 64 : 128, slots = 512;
            auto need = [&](std::size_t rows) { const std::size_t rt = std::max<std::size_t>(1, (rows + 127) / 128); return ((slots + rt - 1) / rt) * bn; };
            // (from the LARGEST local block of the layout, not from mine: every rank must arrive at the same panel grid - the
            // panels are what the all-reduces carry - and local row counts differ by one block remainder between ranks)
            const std::size_t w = std::max(need((std::size_t)Rr_.count(0)), need((std::size_t)Cc_.count(0)));
            panel_ = std::min<std::size_t>(2048, std::max<std::size_t>(256, (w + 255) / 256 * 256));
            // ... but a product must still consist of SEVERAL panels, or nothing of its all-reduce can hide: at most 1 / 2.5 of
            // the filter's block width (nev + nex columns), not below 128.  Found with the single-rank replay of config 5 on
            // 4 x 2 (320 columns, m_loc = 8192: the rule above gives one 512-column panel): against collectives modelled at
            // 50 GB/s T_rank 3.82 s with that panel, 2.84 s with 128 (profiles/r05_replay_cfg5_4x2_panels_modelled.json)
            const std::size_t cap = std::max<std::size_t>(128, ((nevex_ * 2 + 4) / 5 + bn - 1) / bn * bn);
            panel_ = std::min(panel_, cap);
        }
        build_diag_lists();
        build_redistribution();
        {   // on a loopback grid (single-rank replay, chase_hip_grid_create_loopback) the pieces "received" from absent peers are
            // whatever the staging block held: start it from N(0,1) so that they are finite, data-like numbers
            int kind = 0;
            hip_ok(chase_hip_grid_transport(grid_, &kind, nullptr, nullptr), "grid_transport");
            loopback_ = kind == 2;
            if (loopback_ && stage_rows_ > 0)
                hip_ok(chase_hip_fill_normal(ctx_, CP, (int)stage_rows_, (int)nc_, dStage_, (long)stage_rows_, 0, 0, (long)stage_rows_, 99ull), "fill staging");
        }
    }
    ~pChaseHip() override { for (void* p : owned_) chase_hip_free(ctx_, p); }

    // ---- getters -----------------------------------------------------------------------------------------------------
    std::size_t GetN() const override { return N_; }
    std::size_t GetNev() override { return nev_; }
    std::size_t GetNex() override { return nex_; }
    std::size_t GetLanczosIter() override { return lanczosIter_; }
    std::size_t GetNumLanczos() override { return numLanczos_; }
    std::size_t GetRitzvBlockSize() const override { return nc_; }
    R* GetRitzv() override { return ritzv_; }
    R* GetResid() override { return resid_.data(); }
    ConfigT& GetConfig() override { return config_; }
    int get_nprocs() override { return nprow_ * npcol_; }
    int get_rank() override { return myrow_ + mycol_ * nprow_; }
    bool isSym() override { return is_sym_; }
    bool isPseudoHerm() override { return false; }
    bool checkPseudoHermicityEasy() override { return false; }
    // randomized test H^H v == H v on the grid (linalg/internal/mpi/symOrHerm.hpp:46-96): v ~ N(0,1) column-type seeded
    // 1337 + grid row, u = H_loc^H v (all-reduce over the column group), uT = H_loc v_rowtype (all-reduce over the row
    // group), compared elementwise with the reference's absolute 1e-10 after bringing u back to the column-type layout
    bool checkSymmetryEasy() override
    {
        CHASE_PHASE(ctx_, "checkSymmetryEasy");
        flush_swaps(); sync_comm();
        void* blk = nullptr;
        const std::size_t elems = 3 * m_ + 2 * n_;
        int rc = chase_hip_malloc(ctx_, &blk, elems * sizeof(T));
        if (rc) throw HipStatusError(rc, "checkSymmetryEasy workspace");
        int bad = 0;
        try {
            T* v = (T*)blk; T* uT = v + m_; T* ucol = uT + m_; T* v2 = ucol + m_; T* u = v2 + n_;
            std::vector<T> h(m_), hu(m_), hut(m_);
            std::mt19937 gen(1337.0 + myrow_);
            std::normal_distribution<> d;
            for (auto& x : h) x = rnd(d, gen);
            hip_ok(chase_hip_upload_matrix(ctx_, CP, (int)m_, 1, h.data(), (long)m_, v, (long)m_), "upload v");
            redistribute_c2r(v, v2, 1);
            const T* keep = dHbac_; const std::size_t keep_ld = ldhbac_;
            dHbac_ = dH_; ldhbac_ = ldh_;                      // the plain products, whatever the matrix type
            hemm_ptr(true, v, u, 0, 1, T(1), T(0), false);
            hemm_ptr(false, v2, uT, 0, 1, T(1), T(0), false);
            dHbac_ = keep; ldhbac_ = keep_ld;
            redistribute_r2c(u, ucol, 1);
            hip_ok(chase_hip_download_matrix(ctx_, CP, (int)m_, 1, ucol, (long)m_, hu.data(), (long)m_), "download");
            hip_ok(chase_hip_download_matrix(ctx_, CP, (int)m_, 1, uT, (long)m_, hut.data(), (long)m_), "download");
            for (std::size_t i = 0; i < m_; ++i)
                if (!(std::abs(hu[i] - hut[i]) <= 1e-10)) { bad = 1; break; }
        } catch (...) { chase_hip_free(ctx_, blk); throw; }
        chase_hip_free(ctx_, blk);
        coll(chase_hip_grid_agree_max(grid_, &bad));
        is_sym_ = (bad == 0);
        return is_sym_;
    }
    // Completes the Hermitian matrix from ONE stored triangle on the distributed block (linalg/internal/mpi/symOrHerm.hpp:127-320,
    // nccl/symOrHerm.hpp, called from Impl/pchase_gpu/pchase_gpu.hpp:643-647): the triangle `uplo` is kept, the other one
    // zeroed and the diagonal halved, then H += H^H.  The reference needs ScaLAPACK's p?tranc for the transpose and throws
    // without it; here the transpose is two pairwise exchanges with the communicators the grid already has (no world
    // communicator, any transport), block and block-cyclic layouts alike.  With S(r, c) = the global indices whose ROW owner is
    // grid row r and whose COLUMN owner is grid column c, rank (r, c) needs H[S(pr, c), S(r, pc)] from every rank (pr, pc):
    //   hop 1, inside the column groups: (pr, pc) sends its local columns S(r, pc) to (r, pc), all its rows;
    //   hop 2, inside the row groups:    (r, pc) passes on to (r, c) the rows of those pieces that belong to column set c,
    //                                    and (r, c) adds their conjugate transposes into its rows S(r, pc).
    // One-off set-up work (as large as the local block): staging is allocated for the call and released.
    void symOrHermMatrix(char uplo) override
    {
        CHASE_PHASE(ctx_, "symOrHermMatrix");
        if (uplo == 'u') uplo = 'U';
        if (uplo == 'l') uplo = 'L';
        if (uplo != 'U' && uplo != 'L') throw std::invalid_argument("symOrHermMatrix: uplo must be 'U' or 'L'");
        flush_swaps(); sync_comm(); hv_valid_ = false; hs_valid_ = false;
        hip_ok(chase_hip_tri_mask_bc(ctx_, CP, uplo, (int)m_, (int)n_, dH_, (long)ldh_, Rr_.nb, nprow_, myrow_, Cc_.nb, npcol_, mycol_),
               "tri_mask_bc");
        // ---- index sets (host arithmetic over the local indices) ------------------------------------------------------------
        std::vector<std::vector<int>> cols1(nprow_);        // hop 1: my local COLUMNS by the grid row that owns them as rows
        for (long jl = 0; jl < (long)n_; ++jl) cols1[Rr_.owner(Cc_.global(jl, mycol_))].push_back((int)jl);
        std::vector<std::vector<int>> rows_of(npcol_);      // my local ROWS by the grid column that owns them as columns
        for (long il = 0; il < (long)m_; ++il) rows_of[Cc_.owner(Rr_.global(il, myrow_))].push_back((int)il);
        const std::size_t s_mine = cols1[myrow_].size();    // |S(myrow, mycol)|
        if (rows_of[mycol_].size() != s_mine) throw std::logic_error("symOrHermMatrix: inconsistent index sets");
        // hop 2 send side: rows of piece pr (its local rows l, global Rr.global(l, pr)) that go to grid column c2
        std::vector<std::vector<std::vector<int>>> rows2(npcol_, std::vector<std::vector<int>>(nprow_));
        std::vector<int> rowmap;                            // hop 2 receive side: row a of a received piece -> my local column
        for (int pr = 0; pr < nprow_; ++pr)
            for (long l = 0; l < Rr_.count(pr); ++l) {
                const long g = Rr_.global(l, pr);
                const int c2 = Cc_.owner(g);
                rows2[c2][pr].push_back((int)l);
                if (c2 == mycol_) rowmap.push_back((int)Cc_.local(g));
            }
        if (rowmap.size() != n_) throw std::logic_error("symOrHermMatrix: inconsistent row map");
        std::size_t max_cols1 = 0, max_from = 0, max_ncount = 0;
        for (auto& v : cols1) max_cols1 = std::max(max_cols1, v.size());
        for (auto& v : rows_of) max_from = std::max(max_from, v.size());
        for (int c2 = 0; c2 < npcol_; ++c2) max_ncount = std::max(max_ncount, (std::size_t)Cc_.count(c2));
        // ---- staging -------------------------------------------------------------------------------------------------------
        const std::size_t z_elems = N_ * s_mine, pack1 = m_ * max_cols1, psend = max_ncount * s_mine, precv = n_ * max_from;
        std::vector<void*> tmp;
        auto talloc = [&](std::size_t bytes) {
            void* q = nullptr;
            int rc = chase_hip_malloc(ctx_, &q, std::max<std::size_t>(bytes, 16));
            if (rc) throw HipStatusError(rc, "symOrHermMatrix staging");
            tmp.push_back(q);
            return q;
        };
        auto tints = [&](const std::vector<int>& v) {
            int* d = (int*)talloc(std::max<std::size_t>(v.size(), 1) * sizeof(int));
            if (!v.empty()) hip_ok(chase_hip_memcpy_h2d(ctx_, d, v.data(), v.size() * sizeof(int)), "h2d");
            return d;
        };
        try {
            T* Z = (T*)talloc(z_elems * sizeof(T));
            T* buf1 = (T*)talloc(std::max(pack1, psend) * sizeof(T));
            T* buf2 = (T*)talloc(precv * sizeof(T));
            std::vector<std::size_t> zoff(nprow_ + 1, 0);
            for (int pr = 0; pr < nprow_; ++pr) zoff[pr + 1] = zoff[pr] + (std::size_t)Rr_.count(pr) * s_mine;
            // ---- hop 1: column group, partner of step s is (s - me) mod p (an involution: both sides name each other) ------------
            for (int st = 0; st < nprow_; ++st) {
                const int peer = ((st - myrow_) % nprow_ + nprow_) % nprow_;
                const std::vector<int>& cl = cols1[peer];
                int* d_idx = tints(cl);
                hip_ok(chase_hip_cols_indexed(ctx_, CP, (int)m_, dH_, (long)ldh_, buf1, (long)m_, d_idx, (int)cl.size()), "cols_indexed");
                coll(chase_hip_grid_sendrecv(grid_, CHASE_HIP_COL, buf1, m_ * cl.size() * E, peer, Z + zoff[peer],
                                             (std::size_t)Rr_.count(peer) * s_mine * E, peer));
            }
            // ---- hop 2: row group ------------------------------------------------------------------------------------------------
            int* d_rowmap = tints(rowmap);
            for (int st = 0; st < npcol_; ++st) {
                const int peer = ((st - mycol_) % npcol_ + npcol_) % npcol_;
                const std::size_t prow = (std::size_t)Cc_.count(peer);       // rows of the piece I pack for `peer`
                std::size_t roff = 0;
                for (int pr = 0; pr < nprow_; ++pr) {
                    const std::vector<int>& rl = rows2[peer][pr];
                    if (rl.empty() || s_mine == 0) { roff += rl.size(); continue; }
                    int* d_idx = tints(rl);
                    hip_ok(chase_hip_rows_indexed(ctx_, CP, Z + zoff[pr], (long)Rr_.count(pr), buf1 + roff, (long)prow, d_idx,
                                                  (int)rl.size(), (int)s_mine, 0), "rows_indexed");
                    roff += rl.size();
                }
                if (roff != prow) throw std::logic_error("symOrHermMatrix: packed piece has the wrong row count");
                const std::size_t from = rows_of[peer].size();               // |S(myrow, peer)|: columns of what I receive
                coll(chase_hip_grid_sendrecv(grid_, CHASE_HIP_ROW, buf1, prow * s_mine * E, peer, buf2, n_ * from * E, peer));
                int* d_colmap = tints(rows_of[peer]);
                hip_ok(chase_hip_conj_transpose_add(ctx_, CP, (int)n_, (int)from, buf2, (long)n_, d_rowmap, d_colmap, dH_, (long)ldh_),
                       "conj_transpose_add");
            }
            hip_ok(chase_hip_ctx_sync(ctx_), "sync");
        } catch (...) {
            chase_hip_ctx_sync(ctx_);
            for (void* q : tmp) chase_hip_free(ctx_, q);
            throw;
        }
        for (void* q : tmp) chase_hip_free(ctx_, q);
        is_sym_ = true;
    }
    void Sort(R*, R*, R*) override {}
    void ApplyKconjugate(std::size_t) override {}
    void HEMM_H2(std::size_t, T, T, T, std::size_t, std::size_t = 0) override
    {
        throw std::logic_error("pChaseHip: HEMM_H2 belongs to the pseudo-Hermitian Impl");
    }
    void set_early_locked_residuals(std::vector<R> r) override { early_ = std::move(r); }

    // HipImplExtras
    std::size_t locked() const override { return locked_; }
    int last_qr_variant() const override { return last_qr_variant_; }
    double filter_ms() const override { return filter_ms_; }
    std::size_t hemm_calls() const override { return hemm_calls_; }
    std::size_t hemm_reused_vecs() const override { return hemm_reused_vecs_; }
    void set_device_rng(bool f) override { device_rng_ = f; }
    void reset_counters() override
    {
        filter_ms_ = 0; hemm_calls_ = 0; hemm_reused_vecs_ = 0;
        hemm_sp_calls_ = 0; hemm_sp_vecs_ = 0; sp_filters_ = 0; hemm_sp_split_calls_ = 0;
    }
    // mixed-precision filter.  Collective: every rank must hold the same value when a filter call starts (the decision in
    // Shift is taken from the replicated residuals, so equal switches give equal decisions)
    bool set_mixed_precision(bool on) override { mixed_ = on; return true; }
    bool mixed_precision() const override { return mixed_; }
    std::size_t hemm_sp_calls() const override { return hemm_sp_calls_; }
    std::size_t hemm_sp_vecs() const override { return hemm_sp_vecs_; }
    std::size_t sp_filters() const override { return sp_filters_; }
    bool set_sp_product(int v) override { sp_split_ = v != 0; return true; }      // collective, like mixed_precision
    int sp_product() const override { return sp_split_ ? 1 : 0; }
    std::size_t hemm_sp_split_calls() const override { return hemm_sp_split_calls_; }
    void* device_V1() override { flush_swaps(); sync_comm(); return dV1_; }
    std::size_t local_rows() const override { return m_; }
    std::size_t local_cols_h() const { return n_; }
    // (like set_panel_cols: anything in flight is waited for first - an unpipelined product does not wait per panel)
    void set_pipeline(bool f) { flush_swaps(); sync_comm(); pipeline_ = f; }
    bool pipeline() const { return pipeline_; }
    // Run-time knobs of the panel pipeline (first-contact self-tuning of bench.py --gpus N: they cannot be tuned without the
    // hardware the job runs on).  Collective: every rank must set the same value at the same point of its call sequence (the
    // panel grid defines which columns one all-reduce carries).  Anything in flight is waited for first; the per-panel
    // events of the old grid are all complete by then, so a slot index may mean another column range afterwards.
    void set_panel_cols(std::size_t w)
    {
        if (w < 64 || w > 4096 || w % 64) throw std::invalid_argument("panel_cols: a multiple of 64 in [64, 4096]");
        flush_swaps(); sync_comm();
        panel_ = w;
    }
    std::size_t panel_cols() const { return panel_; }
    void set_panel_rounds(int r) { if (r < 0 || r > 16) throw std::invalid_argument("panel_rounds: 0..16"); panel_rounds_ = r; }
    int panel_rounds() const { return panel_rounds_; }
    double last_ortho_check() const { return last_ortho_; }          // CHASE_QR_CHECK_ORTHO: ||Q^H Q - I||_inf of the last Householder QR

    // ---- life cycle ----------------------------------------------------------------------------------------------------
    // (the caller owns H_loc and may have changed it between the solves of a sequence: the fp32 shadow is converted anew)
    void Start() override { locked_ = 0; sp_active_ = false; hs_valid_ = false; }

    // pchase_cpu.hpp:272-311: every grid row seeds mt19937(1337 + coords[0]) and fills its block in memory order
    void initVecs(bool random) override
    {
        CHASE_PHASE(ctx_, "initVecs");
        hv_valid_ = false;
        if (random) {
            if (device_rng_) {
                hip_ok(chase_hip_fill_normal_bc(ctx_, CP, (int)m_, (int)nc_, dV1_, (long)m_, (long)N_, (int)Rr_.nb,
                                                nprow_, myrow_, 1337ull), "fill_normal_bc");
            } else {
                std::vector<T> h(m_ * nc_);
                std::mt19937 gen(1337.0 + myrow_);
                std::normal_distribution<> d;
                for (auto& x : h) x = rnd(d, gen);
                hip_ok(chase_hip_upload_matrix(ctx_, CP, (int)m_, (int)nc_, h.data(), (long)m_, dV1_, (long)m_), "upload V");
            }
        }
        init_vecs_hook(random);
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, (int)nc_, dV1_, (long)m_, dV2_, (long)m_), "lacpy");
        reset_perm();
        next_bAc_ = true;
    }
    // caller-provided start vectors (approximate-solution mode): local m_loc x nevex block, host memory
    void upload_local_V(const T* host, std::size_t ldv)
    {
        hv_valid_ = false;
        hip_ok(chase_hip_upload_matrix(ctx_, CP, (int)m_, (int)nc_, host, (long)ldv, dV1_, (long)m_), "upload V");
    }
    void download_local_V(T* host, std::size_t ldv)
    {
        flush_swaps(); sync_comm();
        hip_ok(chase_hip_download_matrix(ctx_, CP, (int)m_, (int)nc_, dV1_, (long)m_, host, (long)ldv), "download V");
    }
    // pchase_cpu.hpp:313-331: re-randomise the given columns (offset by fixednev) of the local V1 block, mirror to V2
    void ReinitColumns(std::size_t fixednev, std::size_t const* col_indices, std::size_t n_indices) override
    {
        CHASE_PHASE(ctx_, "ReinitColumns");
        if (n_indices == 0) return;
        flush_swaps();
        sync_comm(); hv_valid_ = false;
        std::mt19937 gen(4242.0 + myrow_);                      // pchase_cpu.hpp:313-331: 4242 + grid row
        std::normal_distribution<> d;
        std::vector<T> h(m_);
        for (std::size_t c = 0; c < n_indices; ++c) {
            const std::size_t j = fixednev + col_indices[c];
            if (j >= nc_) throw std::invalid_argument("ReinitColumns: column out of range");
            for (auto& x : h) x = rnd(d, gen);
            hip_ok(chase_hip_upload_matrix(ctx_, CP, (int)m_, 1, h.data(), (long)m_, dV1_ + j * m_, (long)m_), "upload column");
            hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, 1, dV1_ + j * m_, (long)m_, dV2_ + j * m_, (long)m_), "lacpy");
        }
    }

    void End() override { flush_swaps(); sync_comm(); hip_ok(chase_hip_ctx_sync(ctx_), "sync"); }

    // ---- filter --------------------------------------------------------------------------------------------------------
    void FilterPhaseStart() override
    {
        roctx_push("chase:Filter");
        flush_swaps();
        chase_hip_ctx_set_phase(ctx_, 1);
        hip_ok(chase_hip_timer_start(ctx_), "timer");
    }
    void FilterPhaseEnd() override
    {
        sync_comm();
        float ms = 0;
        hip_ok(chase_hip_timer_stop(ctx_, &ms), "timer");
        chase_hip_ctx_set_phase(ctx_, 0);
        filter_ms_ += ms;
        roctx_pop(ctx_);
    }

    // mpi/shiftDiagonal.hpp:21-78 / cuda/shiftDiagonal.cu:100-149: shift the locally owned diagonal entries
    void Shift(T c, bool isunshift = false) override
    {
        hv_shift_ += std::real(c);          // the cached products belong to the unshifted matrix: (H + sI) V = H V + s V
        if (isunshift) next_bAc_ = true;
        hip_ok(chase_hip_shift_list(ctx_, CP, dH_, (long)ldh_, d_diag_rows_, d_diag_cols_, (int)diag_cnt_, std::real(c)),
               "shift_list");
        // mixed precision: decided once per filter call like ChaseHip::Shift, from the residuals the driver left in resid_ -
        // replicated, so every rank decides alike
        if (isunshift) {
            sp_active_ = false;
        } else if (mixed_ && locked_ < nev_ &&
                   *std::min_element(resid_.begin() + locked_, resid_.begin() + nev_) > (R)1e-3) {
            begin_single_precision();
        }
    }
    // a qualifying Shift(-c): the fp32 shadow of the (already shifted) local block.  First time after Start(): the whole block;
    // later filter calls of the solve only changed the diagonal, which is copied from the fp64 block (bitwise what converting
    // the shifted block gives)
    void begin_single_precision()
    {
        if (!sH_) {
            auto pad4 = [](std::size_t r) { return std::max<std::size_t>(4, (r + 3) & ~(std::size_t)3); };   // 16-byte columns
            ld_sh_ = pad4(m_);
            ld_sx_ = pad4(std::max(m_, n_));
            alloc((void**)&sH_, ld_sh_ * std::max<std::size_t>(n_, 1) * sizeof(ST));
            alloc((void**)&sX_, ld_sx_ * nc_ * sizeof(ST));
        }
        if (!hs_valid_) {
            hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)m_, (int)n_, dH_, (long)ldh_, sH_, (long)ld_sh_), "convert_d2s H");
            hs_valid_ = true;
        } else {
            hip_ok(chase_hip_diag_list_d2s(ctx_, CP, dH_, (long)ldh_, sH_, (long)ld_sh_, d_diag_rows_, d_diag_cols_, (int)diag_cnt_),
                   "diag_list_d2s");
        }
        sp_active_ = true;
        sp_counted_ = false;
    }
    // one panel of a filter product on fp32 operands: the input panel is rounded into its columns of the staging block (on the
    // compute stream, after the panel's event wait: the pipeline's ordering is untouched), the product leaves the kernel in fp64
    void product_sp(bool bAc, std::size_t c, std::size_t w, T alpha, const T* in, std::size_t in_ld, T beta, T* out, std::size_t out_ld)
    {
        const std::size_t rows_in = bAc ? m_ : n_, rows_out = bAc ? n_ : m_;
        ST* x = sX_ + c * ld_sx_;
        hip_ok(chase_hip_convert_d2s(ctx_, CP, (int)rows_in, (int)w, in, (long)in_ld, x, (long)ld_sx_), "convert_d2s panel");
        int rc;
        if constexpr (is_cplx<T>::value) {
            const double a[2] = {alpha.real(), alpha.imag()}, b[2] = {beta.real(), beta.imag()};
            rc = (sp_split_ ? chase_hip_gemm_cz_bf16x3 : chase_hip_gemm_cz)(ctx_, bAc ? 'C' : 'N', (int)rows_out, (int)w, (int)rows_in, a,
                                                                            sH_, (long)ld_sh_, x, (long)ld_sx_, b, out, (long)out_ld);
        } else {
            rc = (sp_split_ ? chase_hip_gemm_sd_bf16x3 : chase_hip_gemm_sd)(ctx_, bAc ? 'C' : 'N', (int)rows_out, (int)w, (int)rows_in,
                                                                            alpha, sH_, (long)ld_sh_, x, (long)ld_sx_, beta, out,
                                                                            (long)out_ld);
        }
        hip_ok(rc, "gemm32w");
    }

    void HEMM(std::size_t block, T alpha, T beta, std::size_t offset_left, std::size_t offset_right = 0) override
    {
        flush_swaps();
        const std::size_t ncols = (offset_right < block) ? block - offset_right : 0;
        if (ncols != 0) {
            const std::size_t c0 = locked_ + offset_left;
            if (hv_valid_ && next_bAc_ && beta == T(0) && std::imag(alpha) == 0.0 && c0 >= hv_locked_ &&
                c0 + ncols <= hv_locked_ + hv_block_) {
                // first Chebyshev step on the Ritz vectors RR just produced: the row-type result alpha (H + sI) V is formed
                // from the row-type H V (dW3_) and V (dW1_) that RR left behind - no GEMM, no all-reduce
                T* w1 = dW1_ + c0 * n_;
                if (hv_shift_ != 0.0)
                    hip_ok(chase_hip_scale_rows(ctx_, CP, (int)n_, (int)ncols, w1, (long)n_, 0, hv_shift_), "scale");
                else
                    hip_ok(chase_hip_memset(ctx_, w1, 0, n_ * ncols * sizeof(T)), "memset");
                const double one[2] = {1.0, 0.0};
                hip_ok(chase_hip_memcpy_h2d(ctx_, dPack_, one, sizeof one), "h2d");
                hip_ok(chase_hip_col_axpy(ctx_, CP, (int)n_, (int)ncols, (const double*)dPack_, 0, 0, 1.0, dW3_ + c0 * n_, (long)n_,
                                          w1, (long)n_), "axpy");
                hip_ok(chase_hip_scale_rows(ctx_, CP, (int)n_, (int)ncols, w1, (long)n_, 0, std::real(alpha)), "scale");
                hemm_reused_vecs_ += ncols;
            } else {
                // (the shortcut above, when it applies, has run in fp64 and is no fp32 product)
                hemm_dir(next_bAc_, c0, ncols, alpha, beta, true, sp_active_);
                if (sp_active_) {
                    if (!sp_counted_) { ++sp_filters_; sp_counted_ = true; }
                    ++hemm_sp_calls_;
                    hemm_sp_vecs_ += ncols;
                    if (sp_split_) ++hemm_sp_split_calls_;
                } else {
                    ++hemm_calls_;
                }
            }
        }
        hv_valid_ = false;
        next_bAc_ = !next_bAc_;
    }

    // ---- QR (pchase_cpu.hpp:572-867) -------------------------------------------------------------------------------------
    void QR(std::size_t, R cond) override
    {
        CHASE_PHASE(ctx_, "QR");
        flush_swaps(); sync_comm(); hv_valid_ = false;
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, (int)locked_, dV1_, (long)m_, dV2_, (long)m_), "lacpy");
        int disable = config_.DoCholQR() ? 0 : 1;
        if (const char* s = std::getenv("CHASE_DISABLE_CHOLQR")) disable = std::atoi(s);
        R thld_hi = 1e8, thld_lo = 2e1;
        if (const char* s = std::getenv("CHASE_CHOLQR1_THLD")) thld_lo = std::atof(s);
        last_qr_variant_ = 0;
        if (forced_qr_ >= 0) {                                  // single-rank replay: the recording's variant (set_forced_qr)
            if (forced_qr_ == 0) householder();
            else { last_qr_variant_ = forced_qr_; cholqr_dist(forced_qr_); }
        } else if (disable == 1 && cond != (R)1.0) {
            householder();
        } else {
            const int variant = (cond > thld_hi) ? 3 : (cond < thld_lo ? 1 : 2);
            last_qr_variant_ = variant;
            if (cholqr_dist(variant) != 0) householder();
        }
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, (int)locked_, dV2_, (long)m_, dV1_, (long)m_), "lacpy");
        const std::size_t un = nevex_ - locked_;
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, (int)un, dV1_ + locked_ * m_, (long)m_, dV2_ + locked_ * m_, (long)m_), "lacpy");
    }

    // ---- Rayleigh-Ritz (mpi/rayleighRitz.hpp:103-186 + pchase_cpu.hpp:869-896) ------------------------------------------
    void RR(R* ritzv, std::size_t block) override
    {
        CHASE_PHASE(ctx_, "RR");
        flush_swaps(); sync_comm();
        const std::size_t c0 = locked_;
        // Like the reference (pchase_gpu.hpp:1631-1633), V is re-broadcast inside the row group so that the replicas over the
        // grid columns are bitwise equal when Rayleigh-Ritz starts: QR runs separately in every column group, and two column
        // communicators may sum their Gram matrices in different orders - a last-bit difference that CholQR2 / shifted CholQR
        // amplify by cond(V) eps.  Columns that get locked right after this step are never filtered again, so nothing later
        // would erase it (round 3 dropped the broadcast; the advisor's finding).  0.67 GB inside a 2-GPU row group per call at
        // config 4, a few ms over xGMI.  CHASE_HIP_RR_RESYNC=0 skips it (single-column grids have nothing to agree).
        static const bool resync = [] { const char* e = std::getenv("CHASE_HIP_RR_RESYNC"); return e ? std::atoi(e) != 0 : true; }();
        if (resync && npcol_ > 1) coll(chase_hip_grid_bcast(grid_, CHASE_HIP_ROW, dV1_ + c0 * m_, m_ * block * E, 0, 0));
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, (int)block, dV1_ + c0 * m_, (long)m_, dV2_ + c0 * m_, (long)m_), "lacpy");
        // round 5: the column -> row redistribution of V (its packed broadcasts run inside the COLUMN group, like the product's
        // all-reduces) is ISSUED FIRST: it does not depend on the product, and queued behind the last all-reduce panel (round 4)
        // it was pure exposed time.  Now the broadcasts run beside the first panel's GEMM; the unpack waits for them below.
        redistribute_start(c2r_, CHASE_HIP_COL, myrow_, dV2_ + c0 * m_, m_, block);
        chase_hip_ctx_set_phase(ctx_, 2);                                    // H-times-block product outside the filter
        // panel-pipelined like the filter's products (round 4): the all-reduce of column panel p (1.34 GB in all at config 4 on
        // 4 x 2) runs beside the GEMM of panel p + 1
        hemm_dir(true, c0, block, T(1), T(0), true);                         // W1 = H^H V1 (row-type), all-reduced
        chase_hip_ctx_set_phase(ctx_, 0);
        redistribute_finish(c2r_, dW2_ + c0 * n_, n_, block);                // W2 = V2 in the row-type layout (waits for the streams)
        // A = V^H (H V), Hermitian: only the upper block trapezoid is multiplied, packed and summed over the row group
        hip_ok(chase_hip_herkx(ctx_, CP, (int)block, (int)n_, dW2_ + c0 * n_, (long)n_, dW1_ + c0 * n_, (long)n_, dA_, (long)block, 0), "herkx");
        // Identical Ritz pairs on every rank by identical INPUT (round 5; rounds 2-4 broadcast the 105 MB eigenvector matrix
        // from rank (0,0) after the eigensolver): the packed triangle is summed over the row group - every member of a row
        // group then holds the same bits - and broadcast once from grid row 0 inside the column groups (52 MB at config 4), so
        // that every rank feeds the same matrix to the eigensolver, whose kernels and host stages are deterministic
        // (tests: bitwise equal replicas across ranks).  CHASE_HIP_RR_AGREE=vectors restores the broadcast of the result.
        static const bool agree_vectors = [] { const char* e = std::getenv("CHASE_HIP_RR_AGREE"); return e && std::string(e) == "vectors"; }();
        allreduce_packed_upper(dA_, block, CHASE_HIP_ROW, agree_vectors ? -1 : CHASE_HIP_COL);
        hip_ok(chase_hip_heevd(ctx_, CP, (int)block, dA_, (long)block, ritzv), "heevd");
        if (agree_vectors) agree_vector(ritzv, block, dA_, block * block);
        else rr_guard(ritzv, block);
        hv_valid_ = false;
        if (resd_reuse_) {
            // row-type H V and V of the new Ritz vectors without another HEMM / all-reduce / redistribution:
            // (H^H Q) A and Q A from the row-type blocks this step already holds (the reference recomputes both in
            // residuals(), mpi/residuals.hpp:61-107; equal up to rounding)
            if (!dW3_) alloc((void**)&dW3_, n_ * nc_ * sizeof(T));
            gemm('N', n_, block, block, T(1), dW1_ + c0 * n_, n_, dA_, block, T(0), dW3_ + c0 * n_, n_);
            gemm('N', n_, block, block, T(1), dW2_ + c0 * n_, n_, dA_, block, T(0), dW1_ + c0 * n_, n_);
            hv_valid_ = true; hv_locked_ = locked_; hv_block_ = block; hv_shift_ = 0.0;
        }
        gemm('N', m_, block, block, T(1), dV2_ + c0 * m_, m_, dA_, block, T(0), dV1_ + c0 * m_, m_);
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, (int)block, dV1_ + c0 * m_, (long)m_, dV2_ + c0 * m_, (long)m_), "lacpy");
        // the Ritz VALUES still go round (2560 doubles, behind the back-transformation's launches): they steer every rank's
        // control flow, and a rank whose host LAPACK stage rounded differently must not take another branch
        if (!agree_vectors) agree_vector(ritzv, block, nullptr, 0);
    }

    // ---- residuals (mpi/residuals.hpp:61-107) ----------------------------------------------------------------------------
    void Resd(R* ritzv, R* resd, std::size_t) override
    {
        CHASE_PHASE(ctx_, "Resd");
        flush_swaps(); sync_comm();
        const std::size_t c0 = locked_, sub = nevex_ - locked_;
        const T *HV, *Vr;
        if (hv_valid_ && hv_shift_ == 0.0 && hv_locked_ == locked_ && hv_block_ == sub) {   // left behind by RR
            HV = dW3_ + c0 * n_; Vr = dW1_ + c0 * n_;
        } else {
            redistribute_start(c2r_, CHASE_HIP_COL, myrow_, dV2_ + c0 * m_, m_, sub);   // V2 (== V1) -> row-type, issued first (see RR)
            chase_hip_ctx_set_phase(ctx_, 2);
            hemm_dir(true, c0, sub, T(1), T(0), true);                       // W1 = H^H V1 (panel-pipelined, see RR)
            chase_hip_ctx_set_phase(ctx_, 0);
            redistribute_finish(c2r_, dW2_ + c0 * n_, n_, sub);              // W2 = V2 row-type (waits for the streams)
            HV = dW1_ + c0 * n_; Vr = dW2_ + c0 * n_;
            hv_valid_ = false;                                               // dW1_ no longer holds the cached V
        }
        sum_resid_squares(HV, Vr, ritzv, resd, sub);
        recheck_borderline(ritzv, resd, sub);
        if (resd != resid_.data() + locked_) std::memcpy(resid_.data() + locked_, resd, sub * sizeof(R));
    }

    // out[j] = || HV_j - lambda_j Vr_j ||_2 of row-type blocks: local sums of squares, all-reduce over the row communicator,
    // sqrt (mpi/residuals.hpp:99-105).  Round 5: the sums stay on the device across the all-reduce (nccl/residuals.hpp:28-88
    // does the same) and are made identical on every rank by ONE broadcast from grid row 0 inside the column groups - the
    // members of a row group hold the same bits after their all-reduce -; one read-back instead of three host round trips.
    void sum_resid_squares(const T* HV, const T* Vr, const R* lambda, R* out, std::size_t cnt)
    {
        double* d = (double*)dPack_;
        hip_ok(chase_hip_resid_norms_dev(ctx_, CP, (int)n_, (int)cnt, HV, (long)n_, Vr, (long)n_, lambda, d, 1), "resid_norms");
        coll(chase_hip_grid_allreduce(grid_, CHASE_HIP_ROW, d, cnt, 0));
        coll(chase_hip_grid_bcast(grid_, CHASE_HIP_COL, d, cnt, 0, 0));
        hip_ok(chase_hip_memcpy_d2h(ctx_, out, d, cnt * sizeof(double)), "d2h");
        for (std::size_t i = 0; i < cnt; ++i) out[i] = std::sqrt(out[i]);
    }

    // Lock on what the reference would see (see ChaseHip::recheck_borderline): residuals within 1e-3 of the tolerance are
    // taken again from the reference's residual step as it stands (mpi/residuals.hpp:61-107: fresh four-product H v,
    // column -> row redistribution of v, local sums of squares, all-reduce over the row group) on just those columns.
    // Collective: the residuals were agreed above, so every rank selects the same columns.
    void recheck_borderline(const R* ritzv, R* resd, std::size_t sub)
    {
        static const bool on = [] { const char* e = std::getenv("CHASE_HIP_RESD_RECHECK"); return e ? std::atoi(e) != 0 : true; }();
        if (!on) return;
        const R tol = (R)config_.GetTol();
        // the window is the larger of 1e-3 tol and the rounding gap between the three-product / cached residual and the
        // reference's fresh one (measured at config 4: 0.2 eps ||H||; window 4 eps ||H||, ||H|| from the Lanczos upper bound;
        // independent of tol - the advisor's finding)
        // capped at tol / 2 (round-5 advisor): for ||H|| >= 1e5 tol / eps the rounding-gap term alone would exceed tol and every
        // converged residual would be re-taken in every iteration
        const R window = std::min(std::max((R)1e-3 * tol, (R)4 * std::numeric_limits<R>::epsilon() * norm_h_), (R)0.5 * tol);
        std::vector<std::size_t> idx;
        if (forced_recheck_ >= 0) {                                        // single-rank replay: as many as the recording re-took
            for (std::size_t j = 0; j < std::min<std::size_t>((std::size_t)forced_recheck_, sub); ++j) idx.push_back(j);
        } else {
            for (std::size_t j = 0; j < sub; ++j)
                if (std::abs(resd[j] - tol) <= window) idx.push_back(j);
        }
        const std::size_t k = idx.size();
        if (k == 0) return;
        if (k > 256 || k > nc_) {
            // too many for the scratch: the reference's residual step as it stands on ALL unlocked columns (fresh four-product
            // H V) instead of keeping values the window says may differ from the reference's
            std::vector<R> fresh(sub);
            fresh_residuals(locked_, sub, ritzv, fresh.data());
            std::memcpy(resd, fresh.data(), sub * sizeof(R));
            resd_rechecked_ += sub;
            return;
        }
        if (chk_cols_ < 2 * k) {                                           // row-type scratch: H v and v of the k columns
            const std::size_t cols = (2 * k + 31) / 32 * 32;
            alloc((void**)&dChk_, n_ * cols * sizeof(T));                 // (grow-only; an outgrown block lives until the Impl dies)
            chk_cols_ = cols;
        }
        std::vector<R> lam(k), sq(k);
        for (std::size_t i = 0; i < k; ++i) {
            lam[i] = ritzv[idx[i]];
            hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, 1, dV1_ + (locked_ + idx[i]) * m_, (long)m_, dVt_ + i * m_, (long)m_), "lacpy");
        }
        T* HVr = dChk_;
        T* Vr = dChk_ + k * n_;
        chase_hip_ctx_set_phase(ctx_, 3);
        hemm_ptr(true, dVt_, HVr, 0, k, T(1), T(0), false);
        chase_hip_ctx_set_phase(ctx_, 0);
        redistribute_c2r(dVt_, Vr, k);
        sum_resid_squares(HVr, Vr, lam.data(), sq.data(), k);
        for (std::size_t i = 0; i < k; ++i) resd[idx[i]] = sq[i];
        resd_rechecked_ += k;
    }
    // the reference's residual step as it stands (mpi/residuals.hpp:61-107) on columns [c0, c0 + cnt): fresh four-product H V
    void fresh_residuals(std::size_t c0, std::size_t cnt, const R* lambda, R* out)
    {
        hv_valid_ = false;                                                   // dW1_ / dW2_ are scratch from here on
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, (int)cnt, dV1_ + c0 * m_, (long)m_, dV2_ + c0 * m_, (long)m_), "lacpy");
        chase_hip_ctx_set_phase(ctx_, 3);
        hemm_ptr(true, dV1_ + c0 * m_, dW1_ + c0 * n_, 0, cnt, T(1), T(0), false);
        chase_hip_ctx_set_phase(ctx_, 0);
        redistribute_c2r(dV2_ + c0 * m_, dW2_ + c0 * n_, cnt);
        sum_resid_squares(dW1_ + c0 * n_, dW2_ + c0 * n_, lambda, out, cnt);
    }
    void set_forced_recheck(long k) override { forced_recheck_ = k; }
    void set_forced_qr(int v) override { forced_qr_ = v; }
    std::size_t forced_qr_retries() const override { return forced_qr_retries_; }
    void set_replay_tolerant(bool on) override { replay_tolerant_ = on; }
    std::size_t replay_tolerated() const override { return replay_tolerated_; }
    std::size_t resd_rechecked() const override { return resd_rechecked_; }

    // the reference's residual step as it stands (mpi/residuals.hpp:61-107: H V, column -> row redistribution of V, local
    // sums of squares, all-reduce over the row group) on the first ncols vectors, never from cached products
    void recompute_residuals(std::size_t ncols, const double* lambda, double* out) override
    {
        CHASE_PHASE(ctx_, "recompute_residuals");
        if (ncols > nc_) throw std::invalid_argument("recompute_residuals: more columns than the Impl holds");
        flush_swaps(); sync_comm();
        fresh_residuals(0, ncols, lambda, out);
    }

    void Swap(std::size_t i, std::size_t j) override
    {
        if (i == j) return;
        std::swap(perm_[i], perm_[j]);
        perm_dirty_ = true;
    }
    void Lock(std::size_t k) override { locked_ += k; }

    // ---- Lanczos (mpi/lanczos.hpp:153-370) ---------------------------------------------------------------------------------
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
    void LanczosDos(std::size_t idx, std::size_t m, T* ritzVc) override
    {
        CHASE_PHASE(ctx_, "LanczosDos");
        flush_swaps(); sync_comm(); hv_valid_ = false;
        hip_ok(chase_hip_upload_matrix(ctx_, CP, (int)m, (int)idx, ritzVc, (long)m, dA_, (long)m), "upload ritzV");
        gemm('N', m_, idx, m, T(1), dV1_, m_, dA_, m, T(0), dV2_, m_);
        hip_ok(chase_hip_lacpy(ctx_, CP, (int)m_, (int)m, dV2_, (long)m_, dV1_, (long)m_), "lacpy");
    }

protected:
    virtual void init_vecs_hook(bool) {}            // pseudo-Hermitian Impl: damp the lower block of random start vectors
    static T rnd(std::normal_distribution<>& d, std::mt19937& g)
    {
        if constexpr (is_cplx<T>::value) { const double re = d(g); const double im = d(g); return T(re, im); }
        else return T(d(g));
    }
    void alloc(void** p, std::size_t bytes)
    {
        int rc = chase_hip_malloc(ctx_, p, bytes);
        if (rc) throw HipStatusError(rc, "chase_hip_malloc");
        owned_.push_back(*p);
    }
    int* upload_ints(const std::vector<int>& v)
    {
        int* d = nullptr;
        alloc((void**)&d, std::max<std::size_t>(v.size(), 1) * sizeof(int));
        if (!v.empty()) hip_ok(chase_hip_memcpy_h2d(ctx_, d, v.data(), v.size() * sizeof(int)), "h2d");
        return d;
    }
    static void coll(int rc) { if (rc) throw HipStatusError(rc, "collective"); }
    void sync_comm() { coll(chase_hip_grid_wait(grid_)); }
    void gemm(char op, std::size_t m, std::size_t n, std::size_t k, T alpha, const T* A, std::size_t lda, const T* B,
              std::size_t ldb, T beta, T* C, std::size_t ldc)
    {
        int rc;
        if constexpr (is_cplx<T>::value) {
            const double a[2] = {alpha.real(), alpha.imag()}, b[2] = {beta.real(), beta.imag()};
            rc = chase_hip_gemm_z(ctx_, op, (int)m, (int)n, (int)k, a, A, (long)lda, B, (long)ldb, b, C, (long)ldc);
        } else {
            rc = chase_hip_gemm_d(ctx_, op, (int)m, (int)n, (int)k, alpha, A, (long)lda, B, (long)ldb, beta, C, (long)ldc);
        }
        hip_ok(rc, "gemm");
    }

    // local (row, col) positions of the global diagonal inside this rank's block (pchase_gpu.hpp:340-409)
    void build_diag_lists()
    {
        std::vector<int> rows, cols;
        for (long l = 0; l < Rr_.nloc; ++l) {
            const long g = Rr_.global(l, myrow_);
            if (g < (long)N_ && Cc_.owner(g) == mycol_) { rows.push_back((int)l); cols.push_back((int)Cc_.local(g)); }
        }
        diag_cnt_ = rows.size();
        d_diag_rows_ = upload_ints(rows);
        d_diag_cols_ = upload_ints(cols);
    }

    struct Xfer { int root = 0; int cnt = 0; int* d_src = nullptr; int* d_dst = nullptr; };
    // One packed broadcast per source rank.  c2r (column-type -> row-type) runs inside my column group: every member
    // needs the same row-type block (global rows owned by grid column mycol), gathered from the members' column-type rows.
    void build_redistribution()
    {
        for (int ip = 0; ip < nprow_; ++ip) {
            std::vector<int> src, dst;
            for (long g = 0; g < (long)N_; ++g)
                if (Rr_.owner(g) == ip && Cc_.owner(g) == mycol_) { src.push_back((int)Rr_.local(g)); dst.push_back((int)Cc_.local(g)); }
            Xfer x; x.root = ip; x.cnt = (int)src.size();
            if (x.cnt) { x.d_src = upload_ints(src); x.d_dst = upload_ints(dst); c2r_.push_back(x); }
        }
        for (int jp = 0; jp < npcol_; ++jp) {
            std::vector<int> src, dst;
            for (long g = 0; g < (long)N_; ++g)
                if (Cc_.owner(g) == jp && Rr_.owner(g) == myrow_) { src.push_back((int)Cc_.local(g)); dst.push_back((int)Rr_.local(g)); }
            Xfer x; x.root = jp; x.cnt = (int)src.size();
            if (x.cnt) { x.d_src = upload_ints(src); x.d_dst = upload_ints(dst); r2c_.push_back(x); }
        }
        // global row of every local column-type row, per grid row (Householder fallback gathers the full vectors)
        for (int ip = 0; ip < nprow_; ++ip) {
            std::vector<int> gl((std::size_t)Rr_.count(ip));
            for (std::size_t l = 0; l < gl.size(); ++l) gl[l] = (int)Rr_.global((long)l, ip);
            d_rowmap_.push_back(upload_ints(gl));
            rowmap_cnt_.push_back((int)gl.size());
        }
    }
    // dst (row-type, ld n_) <- src (column-type, ld m_), ncols columns.  The reference issues one broadcast per contiguous run
    // of rows (distMultiVector.hpp:2658-2718); here one packed broadcast per source rank, all of them issued back to back on
    // the communication stream (each into its own piece of the staging block) with ONE wait of the compute stream
    void redistribute_c2r(const T* src, T* dst, std::size_t ncols) { redistribute(c2r_, CHASE_HIP_COL, myrow_, src, m_, dst, n_, ncols); }
    // dst (column-type, ld m_) <- src (row-type, ld n_)
    void redistribute_r2c(const T* src, T* dst, std::size_t ncols) { redistribute(r2c_, CHASE_HIP_ROW, mycol_, src, n_, dst, m_, ncols); }
    void redistribute(const std::vector<Xfer>& plan, int group, int me, const T* src, std::size_t lds, T* dst, std::size_t ldd,
                      std::size_t ncols)
    {
        redistribute_start(plan, group, me, src, lds, ncols);
        redistribute_finish(plan, dst, ldd, ncols);
    }
    // first half: pack my piece, issue every source rank's broadcast on the group's communication stream (asynchronous: the
    // caller may enqueue independent work - RR and Resd put their whole H-times-block product here - before it asks for the
    // result).  The staging block is in use until redistribute_finish.
    void redistribute_start(const std::vector<Xfer>& plan, int group, int me, const T* src, std::size_t lds, std::size_t ncols)
    {
        std::size_t off = 0;
        for (const Xfer& x : plan) {
            T* piece = dStage_ + off;
            if (me == x.root)
                hip_ok(chase_hip_rows_indexed(ctx_, CP, src, (long)lds, piece, x.cnt, x.d_src, x.cnt, (int)ncols, 0), "pack");
            coll(chase_hip_grid_bcast(grid_, group, piece, (std::size_t)x.cnt * ncols * E, x.root, 1));
            off += (std::size_t)x.cnt * ncols;
        }
    }
    // second half: ONE wait of the compute stream for the communication streams, then the scatter into the destination layout
    void redistribute_finish(const std::vector<Xfer>& plan, T* dst, std::size_t ldd, std::size_t ncols)
    {
        sync_comm();
        std::size_t off = 0;
        for (const Xfer& x : plan) {
            hip_ok(chase_hip_rows_indexed(ctx_, CP, dStage_ + off, x.cnt, dst, (long)ldd, x.d_dst, x.cnt, (int)ncols, 1), "unpack");
            off += (std::size_t)x.cnt * ncols;
        }
    }

    // one direction of the distributed HEMM on columns [c0, c0 + nc)  (mpi/hemm.hpp:114-229)
    //   bAc:  W1 = alpha * H_loc^H * V1 + beta' * W1,  beta' = beta on grid row 0 only,  all-reduce over the column group
    //   cAb:  V1 = alpha * H_loc   * W1 + beta' * V1,  beta' = beta on grid col 0 only,  all-reduce over the row group
    void hemm_dir(bool bAc, std::size_t c0, std::size_t nc, T alpha, T beta, bool pipelined, bool sp = false)
    {
        hemm_ptr(bAc, bAc ? dV1_ : dW1_, bAc ? dW1_ : dV1_, c0, nc, alpha, beta, pipelined, sp);
    }
    // in: column-type (bAc) / row-type (cAb) block, out: the other type.  bAc multiplies with dHbac_: H_loc itself for a
    // Hermitian matrix; the pseudo-Hermitian Impl points it at G_loc = S H_loc S (signs of the two off-diagonal quadrants
    // flipped), because H V = S H^H S V (mpi/hemm.hpp:125-199) = G^H V — the reference's four vector sign flips around
    // the conj-transposed GEMM are folded into the matrix once, and the panel pipeline applies unchanged.  cAb is H W.
    // sp (the Hermitian filter while a mixed-precision filter call runs): the local products multiply the fp32 shadow of H_loc
    // with the fp32-rounded input panel and write fp64 - everything else, the all-reduces included, is as without it.
    void hemm_ptr(bool bAc, T* in, T* out, std::size_t c0, std::size_t nc, T alpha, T beta, bool pipelined, bool sp = false)
    {
        const int group = bAc ? CHASE_HIP_COL : CHASE_HIP_ROW;
        const bool root = bAc ? (myrow_ == 0) : (mycol_ == 0);
        const T b = root ? beta : T(0);
        const std::size_t out_ld = bAc ? n_ : m_;
        const std::size_t in_ld = bAc ? m_ : n_;
        const T* Hb = bAc ? dHbac_ : dH_;
        const std::size_t ldb = bAc ? ldhbac_ : ldh_;
        // Two separate questions.  `active`: does THIS direction have a collective (its group has more than one member)?
        // `panels`: is the product cut on the panel grid and ordered by the per-panel events?  It must be whenever EITHER
        // direction's collective runs asynchronously on the communication stream: my input panels are the output of the
        // previous product of the OTHER direction, whose all-reduces may still be in flight - also when my own group has a
        // single member (2 x 1 grid: the row group; round 4 found exactly this with the first real RCCL run between two
        // ranks: the row -> column product read W before the column group's all-reduce had landed).
        const bool active = chase_hip_grid_group_active(grid_, group) != 0;
        const bool other_active = chase_hip_grid_group_active(grid_, bAc ? CHASE_HIP_ROW : CHASE_HIP_COL) != 0;
        const bool pipe = pipelined && pipeline_ && (active || other_active);
        // the panel products run beside the previous panel's all-reduce: finer work units, so that the CUs the collective
        // takes displace a fraction of a tile (chase_hip_ctx_set_gemm_min_rounds; CHASE_HIP_PANEL_ROUNDS, 0 = off)
        const int panel_rounds = panel_rounds_;
        // restored on every way out: hip_ok / coll throw, and a context left in forced K-split mode would give every later
        // product another decomposition (and rounding)
        struct RoundsGuard {
            chase_hip_ctx* ctx;
            RoundsGuard(chase_hip_ctx* c, int r) : ctx(c) { if (c) chase_hip_ctx_set_gemm_min_rounds(c, r); }
            ~RoundsGuard() { if (ctx) chase_hip_ctx_set_gemm_min_rounds(ctx, 0); }
        } rounds_guard(pipe ? ctx_ : nullptr, panel_rounds);
        // the ordering itself lives in panel_pipeline.hpp (and is checked on the CPU against a simulator of streams and events)
        struct Ops {
            pChaseHip* k; bool bAc; int group; T alpha, b; const T* Hb; std::size_t ldb; T* in; std::size_t in_ld; T* out; std::size_t out_ld;
            bool sp;
            void event_wait(int slot) { coll(chase_hip_grid_event_wait(k->grid_, slot)); }
            void product(std::size_t c, std::size_t w)
            {
                if (sp)       k->product_sp(bAc, c, w, alpha, in + c * in_ld, in_ld, b, out + c * out_ld, out_ld);
                else if (bAc) k->gemm('C', k->n_, w, k->m_, alpha, Hb, ldb, in + c * in_ld, in_ld, b, out + c * out_ld, out_ld);
                else     k->gemm('N', k->m_, w, k->n_, alpha, Hb, ldb, in + c * in_ld, in_ld, b, out + c * out_ld, out_ld);
            }
            void allreduce(std::size_t c, std::size_t w, bool async)
            {
                coll(chase_hip_grid_allreduce(k->grid_, group, out + c * out_ld, out_ld * w * E, async ? 1 : 0));
            }
            void event_record(int grp, int slot) { coll(chase_hip_grid_event_record_on(k->grid_, grp, slot)); }
        } ops{this, bAc, group, alpha, b, Hb, ldb, in, in_ld, out, out_ld, sp};
        pipelined_product(ops, pipe, active, group, c0, nc, panel_);
    }
    // X <- S X on the local rows of a column-type / row-type block (global rows >= N/2 change sign)
    void flip_coltype(T* X, std::size_t ncols, double s = -1.0)
    {
        hip_ok(chase_hip_scale_rows_bc(ctx_, CP, (int)m_, (int)ncols, X, (long)m_, (long)(N_ / 2), Rr_.nb, nprow_, myrow_, s), "flip");
    }
    void flip_rowtype(T* X, std::size_t ncols)
    {
        hip_ok(chase_hip_scale_rows_bc(ctx_, CP, (int)n_, (int)ncols, X, (long)n_, (long)(N_ / 2), Cc_.nb, npcol_, mycol_, -1.0), "flip");
    }

    // A (n x n, Hermitian, device) <- sum over `group` of A, moving only the packed upper triangle; agree_group >= 0: the sum
    // is then broadcast from member 0 of that (other) group, so that every rank of the grid holds the same bits
    void allreduce_packed_upper(T* A, std::size_t n, int group, int agree_group = -1)
    {
        hip_ok(chase_hip_pack_upper(ctx_, CP, (int)n, A, (long)n, dPack_), "pack_upper");
        // (both synchronous: the two groups' collectives run on different communication streams, and the compute stream's
        // wait in between is what orders the broadcast behind the sum)
        coll(chase_hip_grid_allreduce(grid_, group, dPack_, n * (n + 1) / 2 * E, 0));
        if (agree_group >= 0) coll(chase_hip_grid_bcast(grid_, agree_group, dPack_, n * (n + 1) / 2 * E, 0, 0));
        hip_ok(chase_hip_unpack_upper(ctx_, CP, (int)n, dPack_, A, (long)n, 1), "unpack_upper");
    }

    // Identical input + deterministic eigensolver = identical Ritz vectors on every rank - by construction, not by check: a
    // rank whose host stages (LAPACK below 384 columns, the leaves and deflation of divide & conquer) run on another CPU or
    // another BLAS threading may round differently, eigenvectors of clustered Ritz values then differ by O(1) rotations
    // between grid rows, and the back-transformed block is inconsistent with NO error raised (round-5 advisor).  So the
    // ranks compare a 64-bit content hash of the eigenvector matrix (one streaming pass over 105 MB at config 4, two
    // 24-double collectives); on any difference the result of rank (0, 0) is broadcast - round 4's always-correct path.
    // CHASE_HIP_RR_GUARD=0 skips the check; CHASE_HIP_RR_GUARD_FAULT=<rank> (tests) flips one bit on that rank first.
    void rr_guard(R* ritzv, std::size_t block)
    {
        static const bool on = [] { const char* e = std::getenv("CHASE_HIP_RR_GUARD"); return e ? std::atoi(e) != 0 : true; }();
        if (!on || nprow_ * npcol_ == 1) return;
        const char* fe = std::getenv("CHASE_HIP_RR_GUARD_FAULT");          // read per call: a test sets it for one solve
        const int fault = fe ? std::atoi(fe) : -1;
        if (fault >= 0 && fault == myrow_ + mycol_ * nprow_) {
            T one;
            hip_ok(chase_hip_memcpy_d2h(ctx_, &one, dA_ + (block / 2) * block + block / 3, sizeof(T)), "d2h");
            one = -one;
            hip_ok(chase_hip_memcpy_h2d(ctx_, dA_ + (block / 2) * block + block / 3, &one, sizeof(T)), "h2d");
        }
        unsigned long long h = 0;
        hip_ok(chase_hip_hash64(ctx_, CP, (int)block, (int)block, dA_, (long)block, &h), "hash64");
        int same = 1;
        coll(chase_hip_grid_agree_equal(grid_, h, &same));
        if (!same) { ++rr_disagreements_; agree_vector(ritzv, block, dA_, block * block); }
    }
    std::size_t rr_disagreements_ = 0;
public:
    std::size_t rr_disagreements() const { return rr_disagreements_; }      // eigensolver results that differed between ranks
protected:

    // make a small host vector (and optionally a device matrix) identical on all ranks: broadcast from grid (0, 0)
    void agree_vector(R* host, std::size_t n, T* dev, std::size_t dev_elems)
    {
        if (!chase_hip_grid_group_active(grid_, CHASE_HIP_ROW) && !chase_hip_grid_group_active(grid_, CHASE_HIP_COL)) return;
        if (n > pack_elems_ * E) throw std::length_error("pChaseHip: agreement scratch too small");
        double* d = (double*)dPack_;
        hip_ok(chase_hip_memcpy_h2d(ctx_, d, host, n * sizeof(double)), "h2d");
        coll(chase_hip_grid_bcast(grid_, CHASE_HIP_COL, d, n, 0, 0));
        coll(chase_hip_grid_bcast(grid_, CHASE_HIP_ROW, d, n, 0, 0));
        hip_ok(chase_hip_memcpy_d2h(ctx_, host, d, n * sizeof(double)), "d2h");
        if (dev && dev_elems) {
            coll(chase_hip_grid_bcast(grid_, CHASE_HIP_COL, dev, dev_elems * E, 0, 0));
            coll(chase_hip_grid_bcast(grid_, CHASE_HIP_ROW, dev, dev_elems * E, 0, 0));
        }
    }

    // mpi/cholqr.hpp:51-397 on the column-type V1 (all nevex columns); returns the agreed potrf info
    int cholqr_dist(int variant)
    {
        const int n = (int)nc_;
        const int passes = variant == 1 ? 1 : (variant == 2 ? 2 : 3);
        int info = 0;
        for (int ps = 0; ps < passes; ++ps) {
            hip_ok(chase_hip_herk(ctx_, CP, n, (int)m_, dV1_, (long)m_, dA_, (long)n), "herk");
            allreduce_packed_upper(dA_, nc_, CHASE_HIP_COL);
            if (variant == 3 && ps == 0) {
                double nrmf = 0;
                hip_ok(chase_hip_abs_trace(ctx_, CP, n, dA_, (long)n, &nrmf), "abs_trace");
                const double shift = std::sqrt((double)N_) * nrmf * std::numeric_limits<double>::epsilon();
                hip_ok(chase_hip_shift_diag(ctx_, CP, n, dA_, (long)n, shift), "shift");
            }
            info = chase_hip_potrf_upper(ctx_, CP, n, dA_, (long)n);
            hip_ok(info, "potrf");
            coll(chase_hip_grid_agree_max(grid_, &info));
            if (info != 0 && forced_qr_ > 0) {
                // replay only: the lone rank's numbers failed a factorisation the recorded solve got through - same passes,
                // same shapes, on a Gram matrix (still packed in dPack_) shifted until it factorises
                // (kept out of the operator log: the real rank has no such retries, everything around them is compared)
                struct Mute { chase_hip_ctx* c; Mute(chase_hip_ctx* x) : c(x) { chase_hip_ctx_oplog_mute(c, 1); } ~Mute() { chase_hip_ctx_oplog_mute(c, -1); } } mute(ctx_);
                double nrmf = 0, boost = 1.0;
                for (int tries = 0; tries < 12 && info != 0; ++tries, boost *= 1e3) {
                    hip_ok(chase_hip_unpack_upper(ctx_, CP, n, dPack_, dA_, (long)n, 1), "unpack_upper");
                    hip_ok(chase_hip_abs_trace(ctx_, CP, n, dA_, (long)n, &nrmf), "abs_trace");
                    if (!(nrmf > 0) || !std::isfinite(nrmf)) nrmf = 1.0;
                    hip_ok(chase_hip_shift_diag(ctx_, CP, n, dA_, (long)n, boost * 1e-10 * nrmf), "shift");
                    info = chase_hip_potrf_upper(ctx_, CP, n, dA_, (long)n);
                    hip_ok(info, "potrf");
                    ++forced_qr_retries_;
                }
                if (info != 0) throw std::runtime_error("pChaseHip: replayed Gram matrix does not factorise even when shifted");
            }
            if (ps == 0 && info != 0) return info;
            hip_ok(chase_hip_trsm_right_upper(ctx_, CP, (int)m_, n, dA_, (long)n, dV1_, (long)m_), "trsm");
        }
        return info;
    }

    // Householder fallback on the row-distributed block (mpi/householder_qr.hpp:737-1417, nccl/householder_qr.hpp:2957):
    // blocked compact-WY panel factorisation inside the column group, pivots in the stacked row order (block and
    // block-cyclic layouts alike), one fused all-reduce per column and two per panel; nothing larger than m_loc x n.
    void householder()
    {
        last_qr_variant_ = 0;
        long off = 0;
        for (int q = 0; q < myrow_; ++q) off += Rr_.count(q);
        coll(chase_hip_houseqr_dist(ctx_, grid_, CHASE_HIP_COL, CP, (int)m_, (int)nc_, dV1_, (long)m_, off));
        // CHASE_QR_CHECK_ORTHO=1 (the reference's diagnostic, linalg/internal/nccl/householder_qr.hpp:214-221,292-372): after the
        // Householder path ||Q^H Q - I||_inf of the distributed Q is computed (Gram matrix, all-reduce over the column group) and
        // reported by the group's first rank; last_ortho_check() returns it
        if (const char* e = std::getenv("CHASE_QR_CHECK_ORTHO")) {
            const std::string v(e);
            if (v == "1" || v == "true" || v == "TRUE" || v == "on" || v == "ON") {
                const std::size_t n = nc_;
                hip_ok(chase_hip_herk(ctx_, CP, (int)n, (int)m_, dV1_, (long)m_, dA_, (long)n), "herk");
                allreduce_packed_upper(dA_, n, CHASE_HIP_COL);
                std::vector<T> G(n * n);
                hip_ok(chase_hip_download_matrix(ctx_, CP, (int)n, (int)n, dA_, (long)n, G.data(), (long)n), "download");
                double inf = 0;
                for (std::size_t i = 0; i < n; ++i) {
                    double row = 0;
                    for (std::size_t j = 0; j < n; ++j) row += std::abs(G[i + j * n] - (i == j ? T(1) : T(0)));
                    inf = std::max(inf, row);
                }
                last_ortho_ = inf;
                if (myrow_ == 0)
                    std::fprintf(stderr, "[ORTHO] ||Q^H Q - I||_inf = %.6e (ncols=%zu, l_rows=%zu)%s\n", inf, n, m_,
                                 inf > 1e-10 ? "\n[ORTHO][WARN] Orthogonality drift above tolerance." : "");
            }
        }
    }
    void reset_perm() { for (std::size_t i = 0; i < nc_; ++i) perm_[i] = (int)i; perm_dirty_ = false; }
    // apply the deferred swaps to V1 and V2 (distMultiVector.hpp:1493 swap_ij acts on both, pchase_cpu.hpp Swap)
    void flush_swaps()
    {
        if (!perm_dirty_) return;
        sync_comm();
        std::vector<int> src, dst;
        for (std::size_t j = 0; j < nc_; ++j)
            if (perm_[j] != (int)j) { src.push_back(perm_[j]); dst.push_back((int)j); }
        if (!src.empty()) {
            hip_ok(chase_hip_permute_cols(ctx_, CP, (int)m_, dV1_, (long)m_, dVt_, (long)m_, src.data(), dst.data(), (int)src.size()), "permute");
            hip_ok(chase_hip_permute_cols(ctx_, CP, (int)m_, dV2_, (long)m_, dVt_, (long)m_, src.data(), dst.data(), (int)src.size()), "permute");
            if (hv_valid_) {     // the cached row-type H V and V follow their vectors (dW2_ is free scratch after RR)
                hip_ok(chase_hip_permute_cols(ctx_, CP, (int)n_, dW3_, (long)n_, dW2_, (long)n_, src.data(), dst.data(), (int)src.size()), "permute");
                hip_ok(chase_hip_permute_cols(ctx_, CP, (int)n_, dW1_, (long)n_, dW2_, (long)n_, src.data(), dst.data(), (int)src.size()), "permute");
            }
        }
        reset_perm();
    }

    // sums of `cnt` device doubles over the column group (dot products / squared norms of column-type vectors)
    void colgroup_sum(double* d, std::size_t cnt) { coll(chase_hip_grid_allreduce(grid_, CHASE_HIP_COL, d, cnt, 0)); }

    void lanczos_core(std::size_t M, std::size_t nv, bool store, R* upperb, R* theta, R* Tau, R* ritzV)
    {
        flush_swaps(); sync_comm(); hv_valid_ = false;
        T *v0, *v1, *v2, *vw;
        double *d_alpha, *d_beta, *d_tmp;
        void* blk = nullptr;
        const std::size_t vec_bytes = (3 * m_ + n_) * nv * sizeof(T);
        const std::size_t sc_bytes = (M * nv * E + M * nv + 2 * nv) * sizeof(double);
        int rc = chase_hip_malloc(ctx_, &blk, vec_bytes + sc_bytes);
        if (rc) throw HipStatusError(rc, "lanczos workspace");
        v0 = (T*)blk; v1 = v0 + m_ * nv; v2 = v1 + m_ * nv; vw = v2 + m_ * nv;
        d_alpha = (double*)(vw + n_ * nv); d_beta = d_alpha + M * nv * E; d_tmp = d_beta + M * nv;
        const int ml = (int)m_, nvi = (int)nv;
        try {
            hip_ok(chase_hip_memset(ctx_, blk, 0, vec_bytes + sc_bytes), "memset");
            hip_ok(chase_hip_lacpy(ctx_, CP, ml, nvi, dV1_, (long)m_, v1, (long)m_), "lacpy");
            // ||v1||: local sums of squares, all-reduce over the column group, sqrt
            sq_norms(v1, nv, d_tmp);
            hip_ok(chase_hip_col_scal(ctx_, CP, ml, nvi, d_tmp, 1, v1, (long)m_), "scal");
            for (std::size_t k = 0; k < M; ++k) {
                if (store)
                    hip_ok(chase_hip_lacpy(ctx_, CP, ml, 1, v1 + (nv - 1) * m_, (long)m_, dV1_ + k * m_, (long)m_), "lacpy");
                // v_w = H^H v1 (row-type) + all-reduce; v2 = redistribute(v_w)
                gemm('C', n_, nv, m_, T(1), dH_, ldh_, v1, m_, T(0), vw, n_);
                coll(chase_hip_grid_allreduce(grid_, CHASE_HIP_COL, vw, n_ * nv * E, 0));
                redistribute_r2c(vw, v2, nv);
                double* ak = d_alpha + k * nv * E;
                hip_ok(chase_hip_col_dot(ctx_, CP, ml, nvi, v1, (long)m_, v2, (long)m_, ak), "dot");
                colgroup_sum(ak, nv * E);
                hip_ok(chase_hip_col_axpy(ctx_, CP, ml, nvi, ak, 0, 1, -1.0, v1, (long)m_, v2, (long)m_), "axpy");
                if (k > 0)
                    hip_ok(chase_hip_col_axpy(ctx_, CP, ml, nvi, d_beta + (k - 1) * nv, 1, 1, -1.0, v0, (long)m_, v2, (long)m_), "axpy");
                sq_norms(v2, nv, d_beta + k * nv);
                if (k == M - 1) break;
                hip_ok(chase_hip_col_scal(ctx_, CP, ml, nvi, d_beta + k * nv, 1, v2, (long)m_), "scal");
                T* t = v0; v0 = v1; v1 = v2; v2 = t;
            }
            if (store) hip_ok(chase_hip_lacpy(ctx_, CP, ml, nvi, v1, (long)m_, dV1_, (long)m_), "lacpy");
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
                const int rc_stemr = chase_hip_stemr_host((int)M, d.data(), e.data(), w.data(), Z.data(), (int)M);
                if (rc_stemr != 0 && replay_tolerant_) {                    // replay: the tape's numbers are what the driver reads
                    std::fill(w.begin(), w.end(), 0.0); std::fill(Z.begin(), Z.end(), 0.0); ++replay_tolerated_;
                } else hip_ok(rc_stemr, "stemr");
                for (std::size_t k = 0; k < M; ++k) {
                    theta[k + i * M] = w[k];
                    if (Tau) Tau[k + i * M] = std::abs(Z[k * M]) * std::abs(Z[k * M]);
                }
                if (ritzV) std::memcpy(ritzV, Z.data(), M * M * sizeof(double));
                const R cand = std::max(std::abs(w[0]), std::abs(w[M - 1])) + std::abs(h_beta[(M - 1) * nv + i]);
                ub = (i == 0) ? cand : std::max(ub, cand);
            }
            // identical bounds / Ritz data on every rank (they steer the whole iteration)
            std::vector<R> pack;
            pack.push_back(ub);
            pack.insert(pack.end(), theta, theta + M * nv);
            if (Tau) pack.insert(pack.end(), Tau, Tau + M * nv);
            if (ritzV) pack.insert(pack.end(), ritzV, ritzV + M * M);
            agree_vector(pack.data(), pack.size(), nullptr, 0);
            std::size_t o = 0;
            ub = pack[o++];
            std::memcpy(theta, pack.data() + o, M * nv * sizeof(R)); o += M * nv;
            if (Tau) { std::memcpy(Tau, pack.data() + o, M * nv * sizeof(R)); o += M * nv; }
            if (ritzV) std::memcpy(ritzV, pack.data() + o, M * M * sizeof(R));
            *upperb = ub;
            norm_h_ = std::abs(ub);
        } catch (...) {
            if (blk) chase_hip_free(ctx_, blk);
            throw;
        }
    }
    // out[j] = ||x_j||_2 of column-type vectors: local sum of squares, column-group all-reduce, sqrt (all on device)
    void sq_norms(const T* x, std::size_t nv, double* out)
    {
        hip_ok(chase_hip_col_sumsq(ctx_, CP, (int)m_, (int)nv, x, (long)m_, out), "sumsq");
        colgroup_sum(out, nv);
        hip_ok(chase_hip_sqrt_inplace(ctx_, out, (int)nv), "sqrt");
    }

    chase_hip_ctx* ctx_;
    chase_hip_grid* grid_;
    std::size_t N_, nev_, nex_, nevex_, nc_;
    T* dH_; std::size_t ldh_;
    const T* dHbac_ = nullptr; std::size_t ldhbac_ = 0;      // matrix of the column->row product (see hemm_ptr)
    R* ritzv_;
    ConfigT config_;
    std::vector<R> resid_, early_;
    std::vector<int> perm_;
    bool perm_dirty_ = false;
    int nprow_ = 1, npcol_ = 1, myrow_ = 0, mycol_ = 0;
    Dim Rr_, Cc_;
    std::size_t m_ = 0, n_ = 0;
    std::size_t locked_ = 0, lanczosIter_ = 0, numLanczos_ = 0;
    std::size_t panel_ = 256;
    int panel_rounds_ = [] { const char* e = std::getenv("CHASE_HIP_PANEL_ROUNDS"); return e ? std::atoi(e) : 4; }();
    bool next_bAc_ = true, device_rng_ = false, pipeline_ = true, pseudo_ = false, is_sym_ = true;
    bool hv_valid_ = false, resd_reuse_ = std::getenv("CHASE_HIP_RESD_REUSE") ? std::atoi(std::getenv("CHASE_HIP_RESD_REUSE")) != 0 : true;
    std::size_t hv_locked_ = 0, hv_block_ = 0, hemm_reused_vecs_ = 0;
    double hv_shift_ = 0.0;
    T* dW3_ = nullptr;
    T* dChk_ = nullptr; std::size_t chk_cols_ = 0, resd_rechecked_ = 0;   // scratch of recheck_borderline
    long forced_recheck_ = -1;                                            // set_forced_recheck (single-rank replay)
    int forced_qr_ = -1; std::size_t forced_qr_retries_ = 0;              // set_forced_qr (single-rank replay)
    bool replay_tolerant_ = false; std::size_t replay_tolerated_ = 0;     // set_replay_tolerant (pseudo-Hermitian replay)
    double last_ortho_ = -1.0;                                            // CHASE_QR_CHECK_ORTHO
    R norm_h_ = 0;                                                        // Lanczos upper bound of the last solve (recheck window)
    bool loopback_ = false; std::size_t stage_rows_ = 0;
    T *dV1_ = nullptr, *dV2_ = nullptr, *dVt_ = nullptr, *dW1_ = nullptr, *dW2_ = nullptr, *dA_ = nullptr;
    T *dPack_ = nullptr, *dStage_ = nullptr;
    std::size_t pack_elems_ = 0;
    int *d_diag_rows_ = nullptr, *d_diag_cols_ = nullptr;
    std::size_t diag_cnt_ = 0;
    std::vector<Xfer> c2r_, r2c_;
    std::vector<int*> d_rowmap_;
    std::vector<int> rowmap_cnt_;
    std::vector<void*> owned_;
    double filter_ms_ = 0;
    std::size_t hemm_calls_ = 0;
    // mixed precision: fp32 shadow of H_loc and the staging block of the input panels (allocated on the first qualifying filter
    // call), their state and counters
    bool mixed_ = false, sp_active_ = false, sp_counted_ = false, hs_valid_ = false;
    ST *sH_ = nullptr, *sX_ = nullptr;
    std::size_t ld_sh_ = 0, ld_sx_ = 0, hemm_sp_calls_ = 0, hemm_sp_vecs_ = 0, sp_filters_ = 0, hemm_sp_split_calls_ = 0;
    bool sp_split_ = false;                // sp_product = 1: the fp32 filter products run as bf16x3
    int last_qr_variant_ = 0;
};

} // namespace chase_amd
