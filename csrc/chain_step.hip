// Chained HyperLSTM backward step: the dR_hyp W_y^T product of step t + 1
// and the main LayerNorm cell backward rows of step t in ONE launch
// (ops/hyper.py).
//
//   [d[h | hh] = dR_hyp W_y^T of step t + 1   (producers: 144 tiles, 8 waves)]
//   [main cell rows of step t                 (512 threads: every operand but
//                                              the d[h] slabs -- ~90 % of the
//                                              row's ~300 KB -- is loaded
//                                              BEFORE the wait)]
//
// The main-cell backward (one 512-thread workgroup per row, csrc/row_cell.h)
// is bound by one CU's streaming rate; its dh input is the only operand the
// small W_y^T product produces. So the rows stream their saves, modulation
// vectors and LayerNorm parameters while the product computes, wait on the
// launch's arrival counter, then read the four d[h] slabs: one launch and one
// kernel boundary fewer per backward step, the row's load phase overlapped
// (profiles/r5: 21.6 -> 15.7 us per step). Reference recurrence:
// /root/reference model.py:66-95.
//
// (Measured and not adopted, round 5: the same chaining for the hyper cell
// -- forward beside R_main after R_hyp, backward beside dR_main W_h^T after
// dvec P^T. Their producers are big enough that sharing the chip with the
// independent product delayed them, and the cell, more than the saved
// boundary: forward 17.57 vs 17.59 us, backward 28.0 vs 20.1 us per step.)
//
// Synchronisation (csrc/handoff.h, chain_*): producer tiles store their
// split-K slabs write-through (sc1), drain and add 1 to the launch's
// arrival counter; a row polls the counter from one lane (bounded; a
// timeout sets *err, which the trainers raise on), joins a barrier and reads
// the slabs with sc1 loads. Producers have the lowest workgroup ids and
// never wait, and workgroups are dispatched in id order, so every producer
// is resident or finished when a row that waits on it is dispatched.
// Counters rotate (chain_rotate): no reset launch per call.
#include "row_cell.h"
#include "skinny_tile.h"

namespace {

constexpr int kNs = 3;    // LDS ring depth of the tiles (the grouped launches' setting)
constexpr int kBn = 64;   // N-tile width

// VEC: the tile's 16-byte write-through epilogue (csrc/skinny_tile.h). On for the
// HyperLSTM backward chain (16.65 -> 16.50 us per launch); off for the
// LayerNorm-LSTM chains, where it measured slower than the dword stores
// (vae_layernorm 8.94 / 8.95 vs 8.80 / 8.80 ms/step, profiles/r16/stores/ab.log).
template <int NW, bool VEC>
__device__ __forceinline__ void producer_tile(const GemmGroup& g, const ChainSync& cs, __hip_bfloat16* smem) {
    if (blockIdx.x == 0) chain_rotate(cs.counters, cs.n, cs.k);
    group_tile<kBn, kNs, NW, skr::ST_WT, VEC>(g, blockIdx.x, smem);
    chain_arrive(cs.counters + cs.k);
}

// backward, main cell: [producers (dR_hyp W_y^T of step t + 1), 8 waves][main cell rows of step t]
// CL = 2: each row on two workgroups (1024 units each: waves 0-3 of the
// 512-thread workgroup; waves 4-7 end at once -- a barrier waits only on the
// waves still running), the two LayerNorm-backward row sums exchanged
// in-launch (row_bwd_body CL): half of the row's ~300 KB of loads per CU.
template <int CL>
__global__ __launch_bounds__(512) void chain_bwd_main_kernel(const GemmGroup g, const int nprod, const skr::BwdArgs cell,
                                                             const ChainSync cs) {
    extern __shared__ __attribute__((aligned(16))) __hip_bfloat16 smem[];
    const int id = blockIdx.x;
    if (id < nprod) {
        producer_tile<8, true>(g, cs, smem);
        return;
    }
    if constexpr (CL == 1) {
        row_bwd_body<512, 4, true, 1, true>(cell, id - nprod, cs.counters + cs.k, (uint32_t)nprod, cs.err);
    } else {
        if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 512 / CL) return;   // (wave-uniform)
        const int r = id - nprod;
        row_bwd_body<512 / CL, 4, true, 1, true, CL>(cell, r / CL, cs.counters + cs.k, (uint32_t)nprod, cs.err, r % CL);
    }
}

// ---- LayerNorm-LSTM chained steps (ops/recurrent.py) ----------------------------------
// forward: [h_{t-1} W_h tiles -> R slabs][cell rows of step t]; backward:
// [dG_{t+1} W_h^T tiles -> dh slabs][cell backward rows of step t]. One row
// per workgroup: NTR = H / 4 threads (waves past NTR / 64 end at once), every
// load but the slabs issued before the in-launch wait (row_fwd_body /
// row_bwd_body CHAIN); the arithmetic of the row kernels (csrc/row_cell.hip).
// probe (skr_chain_ln_set_probe; outputs WRONG while set): 1 the rows end at
// once (producers only), 2 the producers only arrive (rows only, no GEMM).
template <int NTR, int DS>
__global__ __launch_bounds__(512) void chain_ln_fwd_kernel(const GemmGroup g, const int nprod, const skr::FwdArgs cell,
                                                           const ChainSync cs, const int probe) {
    extern __shared__ __attribute__((aligned(16))) __hip_bfloat16 smem[];
    const int id = blockIdx.x;
    if (id < nprod) {
        if (probe == 2) {
            if (blockIdx.x == 0) chain_rotate(cs.counters, cs.n, cs.k);
            chain_arrive(cs.counters + cs.k);
            return;
        }
        producer_tile<8, false>(g, cs, smem);
        return;
    }
    if (probe == 1 || __builtin_amdgcn_readfirstlane(threadIdx.x) >= NTR) return;   // (wave-uniform)
    row_fwd_body<NTR, 4, 0, DS, true>(cell, id - nprod, cs.counters + cs.k, (uint32_t)nprod, cs.err);
}

template <int NTR>
__global__ __launch_bounds__(512) void chain_ln_bwd_kernel(const GemmGroup g, const int nprod, const skr::BwdArgs cell,
                                                           const ChainSync cs, const int probe) {
    extern __shared__ __attribute__((aligned(16))) __hip_bfloat16 smem[];
    const int id = blockIdx.x;
    if (id < nprod) {
        if (probe == 2) {
            if (blockIdx.x == 0) chain_rotate(cs.counters, cs.n, cs.k);
            chain_arrive(cs.counters + cs.k);
            return;
        }
        producer_tile<8, false>(g, cs, smem);
        return;
    }
    if (probe == 1 || __builtin_amdgcn_readfirstlane(threadIdx.x) >= NTR) return;
    row_bwd_body<NTR, 4, false, 1, true>(cell, id - nprod, cs.counters + cs.k, (uint32_t)nprod, cs.err);
}

template <typename K>
void lds_attr(K k, size_t lds) {
    static bool done = false;   // per instantiation, once (never during a graph capture's second call)
    if (!done) {
        (void)hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        done = true;
    }
}

constexpr size_t kLds = (size_t)kNs * (skr::BM + kBn) * skr::BK * 2;

// Group of n problems, the first nprod of which are producers; returns the
// producer tile count (> 0) or a negative code.
int build_group(const GemmProblem* probs, int n, int nprod, GemmGroup& g) {
    if (n < 1 || n > kMaxGroup || nprod < 1 || nprod > n) return -2;
    g = GemmGroup{};
    g.n = n;
    g.start[0] = 0;
    for (int i = 0; i < n; ++i) {
        const int rc = check_problem64(probs[i]);
        if (rc) return rc;
        g.p[i] = probs[i];
        g.start[i + 1] = g.start[i] + (probs[i].N / kBn) * probs[i].splits * row_blocks_of(probs[i].M);
    }
    for (int i = n + 1; i <= kMaxGroup; ++i) g.start[i] = g.start[n];
    return g.start[nprod];
}

int check_sync(const ChainSync* cs) {
    if (cs == nullptr || cs->counters == nullptr || cs->err == nullptr || cs->n < 2 || cs->k < 0 || cs->k >= cs->n)
        return -6;
    return 0;
}

}  // namespace

// Backward main-cell chain: probs[0 .. n) (all producers) produce the row's
// dh_rec slabs (<= 8); everything else as skr_row_bwd_step mod 2 with
// H = 2048 (512 threads x 4 units) and a single dh_out slab; cell->cluster
// == 2 splits every row over two workgroups (exchange buffer cell->part).
SKR_API int skr_chain_bwd_main(const GemmProblem* probs, int n, const skr::BwdArgs* cell, const ChainSync* cs,
                               hipStream_t s) {
    if (cell == nullptr || check_sync(cs)) return -6;
    const skr::BwdArgs& a = *cell;
    if (a.H != 2048 || a.dh_rec == nullptr || a.dhr_nslab < 1 || a.dhr_nslab > 8) return -2;
    if (a.dh_out && a.dho_nslab != 1) return -2;
    const int rc = row_bwd_check(a, 2);
    if (rc) return rc;
    GemmGroup g;
    const int np = build_group(probs, n, n, g);
    if (np < 0) return np;
    // cell.cluster == 2: two workgroups per row (a.part / a.err: the exchange buffer, [2][B][2][16])
    const int cl = a.cluster == 2 ? 2 : 1;
    if (cl == 2 && (a.part == nullptr || a.err == nullptr)) return -6;
    if (cl == 2) {
        lds_attr(chain_bwd_main_kernel<2>, kLds);
        hipLaunchKernelGGL((chain_bwd_main_kernel<2>), dim3(np + a.B * 2), dim3(512), kLds, s, g, np, a, *cs);
    } else {
        lds_attr(chain_bwd_main_kernel<1>, kLds);
        hipLaunchKernelGGL((chain_bwd_main_kernel<1>), dim3(np + a.B), dim3(512), kLds, s, g, np, a, *cs);
    }
    return SKR_CHECK_LAUNCH();
}

SKR_API int skr_chain_sync_size() { return (int)sizeof(ChainSync); }

static int g_chain_ln_probe = 0;

// Timing probes of the chained LayerNorm-LSTM steps (scripts/micro/ln_probe.py;
// outputs WRONG while set): 1 producers only, 2 rows only. Returns the previous.
SKR_API int skr_chain_ln_set_probe(int p) {
    const int prev = g_chain_ln_probe;
    if (p >= 0) g_chain_ln_probe = p;
    return prev;
}

// LayerNorm-LSTM forward step chained: probs (all producers) write the R
// slabs (cell->R, <= 8) the rows of this step sum; rows as skr_row_fwd_step
// mod 0 with H in {256, 512, 1024, 2048}. Returns -2 / -3 / -4 when not taken.
SKR_API int skr_chain_ln_fwd(const GemmProblem* probs, int n, const skr::FwdArgs* cell, const ChainSync* cs,
                             hipStream_t s) {
    if (cell == nullptr || check_sync(cs)) return -6;
    const skr::FwdArgs& a = *cell;
    if (a.B <= 0) return 0;
    if (a.H % 256 != 0 || a.H > 2048 || a.R_nslab < 1 || a.R_nslab > 8 || a.grp_rows > 0) return -2;
    const int rc = row_fwd_check(a, 0);
    if (rc) return rc;
    GemmGroup g;
    const int np = build_group(probs, n, n, g);
    if (np < 0) return np;
    const int ntr = a.H / 4, ds = a.R_nslab <= 1 ? 1 : a.R_nslab <= 2 ? 2 : a.R_nslab <= 4 ? 4 : 8;
    const void* k = nullptr;
#define SKR_CLF(NTR_, DS_) if (ntr == NTR_ && ds == DS_) k = (const void*)chain_ln_fwd_kernel<NTR_, DS_>;
#define SKR_CLF_DS(NTR_) SKR_CLF(NTR_, 1) SKR_CLF(NTR_, 2) SKR_CLF(NTR_, 4) SKR_CLF(NTR_, 8)
    SKR_CLF_DS(64) SKR_CLF_DS(128) SKR_CLF_DS(256) SKR_CLF_DS(512)
#undef SKR_CLF_DS
#undef SKR_CLF
    if (k == nullptr) return -2;
    static const void* attr_done[16];
    static int n_attr = 0;
    bool done = false;
    for (int i = 0; i < n_attr; ++i) done |= attr_done[i] == k;
    if (!done && n_attr < 16) {
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds);
        attr_done[n_attr++] = k;
    }
    int npv = np, prb = g_chain_ln_probe;
    void* args[] = {(void*)&g, (void*)&npv, (void*)&a, (void*)cs, (void*)&prb};
    if (hipLaunchKernel(k, dim3(np + a.B), dim3(512), args, kLds, s) != hipSuccess) return -1;
    return SKR_CHECK_LAUNCH();
}

// LayerNorm-LSTM backward step chained: probs (all producers) write the dh_rec
// slabs (cell->dh_rec, <= 8) of this step's rows; rows as skr_row_bwd_step
// mod 0 with a single dh_out slab (or none).
SKR_API int skr_chain_ln_bwd(const GemmProblem* probs, int n, const skr::BwdArgs* cell, const ChainSync* cs,
                             hipStream_t s) {
    if (cell == nullptr || check_sync(cs)) return -6;
    const skr::BwdArgs& a = *cell;
    if (a.B <= 0) return 0;
    if (a.H % 256 != 0 || a.H > 2048 || a.dh_rec == nullptr || a.dhr_nslab < 1 || a.dhr_nslab > 8 ||
        a.dh_rec2 != nullptr || a.grp_rows > 0)
        return -2;
    if (a.dh_out && a.dho_nslab != 1) return -2;
    const int rc = row_bwd_check(a, 0);
    if (rc) return rc;
    GemmGroup g;
    const int np = build_group(probs, n, n, g);
    if (np < 0) return np;
    const int ntr = a.H / 4;
    const void* k = ntr == 64 ? (const void*)chain_ln_bwd_kernel<64> : ntr == 128 ? (const void*)chain_ln_bwd_kernel<128>
                  : ntr == 256 ? (const void*)chain_ln_bwd_kernel<256> : (const void*)chain_ln_bwd_kernel<512>;
    static const void* attr_done[4];
    static int n_attr = 0;
    bool done = false;
    for (int i = 0; i < n_attr; ++i) done |= attr_done[i] == k;
    if (!done && n_attr < 4) {
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLds);
        attr_done[n_attr++] = k;
    }
    int npv = np, prb = g_chain_ln_probe;
    void* args[] = {(void*)&g, (void*)&npv, (void*)&a, (void*)cs, (void*)&prb};
    if (hipLaunchKernel(k, dim3(np + a.B), dim3(512), args, kLds, s) != hipSuccess) return -1;
    return SKR_CHECK_LAUNCH();
}
