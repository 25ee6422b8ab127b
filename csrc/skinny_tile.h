// One [M <= 128, BN] output tile of the skinny split-K GEMM and the grouped
// launch's workgroup -> (problem, row block, split, N tile) map, shared by
// csrc/skinny_gemm.hip (plain and grouped launches) and csrc/chain_step.hip
// (grouped launches whose producer tiles publish to waiting cell rows).
#pragma once
#include "common.h"
#include "glds_mma.h"
#include "store_policy.h"

// One product of a grouped launch: C_s = A[:, Ks] . Bt[:, Ks]^T, S = splits
// fp32 partial slabs (c_slab apart). Mirrored by sketch_rnn_amd/ops/_hipapi.py.
struct GemmProblem {
    const void* A; int64_t lda;
    const void* Bt; int64_t ldb;
    float* C; int64_t ldc; int64_t c_slab;
    int M, N, K, splits;
};

namespace {

typedef __attribute__((ext_vector_type(4))) float tile_f32x4;

constexpr int kMaxGroup = 4;
struct GemmGroup {
    GemmProblem p[kMaxGroup];
    int start[kMaxGroup + 1];
    int n;
};

// (row block, split, N tile) of workgroup `local` of a problem: row blocks of
// 128 rows outermost, then splits, then N tiles
struct TileIdx { int rb, rows, split, nt; };
__device__ __forceinline__ TileIdx tile_idx(int local, int M, int N, int splits, int bn) {
    const int ntiles = N / bn, per_rb = ntiles * splits;
    TileIdx t;
    t.rb = local / per_rb;
    const int rem = local - t.rb * per_rb;
    t.split = rem / ntiles;
    t.nt = rem - t.split * ntiles;
    t.rows = min(skr::BM, M - t.rb * skr::BM);
    return t;
}

__host__ __device__ constexpr int row_blocks_of(int M) { return M <= skr::BM ? 1 : (M + skr::BM - 1) / skr::BM; }

template <typename P>
__device__ __forceinline__ int64_t split_off(const P& p, const TileIdx& t) {
    return (int64_t)t.split * p.c_slab + (int64_t)t.rb * skr::BM * p.ldc;
}

// In-quad 4 x 4 transpose of one 16 x 16 MFMA accumulator. Before: lane l holds
// column l & 15, rows 4 (l >> 4) + e in v[e]. After: it holds row
// 4 (l >> 4) + (l & 3), columns 4 ((l & 15) >> 2) + e. Two DPP exchange
// rounds (lane ^ 1, lane ^ 2) of two registers each; values only move. Every
// lane must be active.
__device__ __forceinline__ void quad_transpose(float (&v)[4], const int lane) {
    const bool o1 = lane & 1, o2 = lane & 2;
    float x = skr::dpp_f32<0xB1>(o1 ? v[0] : v[1]), y = skr::dpp_f32<0xB1>(o1 ? v[2] : v[3]);
    v[0] = o1 ? x : v[0]; v[1] = o1 ? v[1] : x;
    v[2] = o1 ? y : v[2]; v[3] = o1 ? v[3] : y;
    x = skr::dpp_f32<0x4E>(o2 ? v[0] : v[2]); y = skr::dpp_f32<0x4E>(o2 ? v[1] : v[3]);
    v[0] = o2 ? x : v[0]; v[2] = o2 ? v[2] : x;
    v[1] = o2 ? y : v[1]; v[3] = o2 ? v[3] : y;
}

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const __hip_bfloat16 l = skr::to_bf16(lo), h = skr::to_bf16(hi);
    return (uint32_t)__builtin_bit_cast(uint16_t, l) | ((uint32_t)__builtin_bit_cast(uint16_t, h) << 16);
}

// The tile: glds_mma's accumulators stored to C (fp32, or bf16 with CBF16)
// under store policy ST (csrc/store_policy.h).
//
// Vector epilogue (C 16-byte aligned, ldc a multiple of 4 floats / 8 bf16):
// each accumulator goes through quad_transpose, then a lane stores 4
// consecutive fp32 columns of one row with one 16-byte store (a store
// instruction covers 16 rows x 64 B, where the MFMA layout's dword stores
// cover 4 rows x 64 B with four times the instructions). bf16: the lane's 4
// columns are packed, and lane pairs 4 apart trade halves of two neighbouring
// accumulators so each stores 8 consecutive columns. The buffer descriptor
// ends at the tile's last byte; the row mask alone decides what is stored.
//
// Scalar epilogue (any other destination): one dword / one bf16 per lane in
// MFMA layout. ST_WT there: relaxed agent-scope atomic stores
// (global_store_dword / _short ... sc1). The value is copied out of the accumulator
// vector first: __builtin_bit_cast of an ext-vector ELEMENT (acc[i][j][e])
// reads element 0 for every e on ROCm 7.2 (measured: rows 1-3 of every
// 4-row accumulator group held row 0's values).
//
// ST_WT is also what the chained launches' producers need for their
// in-launch hand-off (csrc/chain_step.hip; CDNA4 guide, hand-off table row 1).
// VEC = false: the scalar epilogue whatever the destination (the chained
// LayerNorm-LSTM producers, measured slower with the vector one).
template <int BN, int NS, bool CBF16 = false, int NW = 4, int ST = skr::ST_PLAIN, bool VEC = true>
__device__ __forceinline__ void glds_tile(const __hip_bfloat16* __restrict__ A, int64_t lda,
                                          const __hip_bfloat16* __restrict__ Bt, int64_t ldb,
                                          void* __restrict__ Cv, int64_t ldc, int M, int n0, int64_t k0, int kslice,
                                          __hip_bfloat16* smem) {
    constexpr int NJ = skr::glds_nj<BN, NW>();
    static_assert(NJ % 2 == 0, "glds_tile: the bf16 epilogue pairs accumulators");
    tile_f32x4 acc[2][NJ];
    skr::glds_mma<BN, NS, NW>(A, lda, Bt, ldb, M, n0, k0, kslice, smem, acc);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wr = w % 4, c0 = n0 + (w / 4) * NJ * 16;
    const int fr = lane & 15, fq = lane >> 4;
    constexpr int ES = CBF16 ? 2 : 4;                       // bytes per element
    // (the last row's byte offset must fit the descriptor's 32-bit offsets)
    const bool vec = VEC && (((uintptr_t)Cv & 15) | (ldc & (16 / ES - 1))) == 0 && ldc < (1 << 22);
    if (vec) {
        const __amdgpu_buffer_rsrc_t r = skr::rsrc(Cv, ((int64_t)(M - 1) * ldc + n0 + BN) * ES);
        const int fc = fr >> 2;                              // column quad of the lane after the transpose
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = 32 * wr + 16 * i + fq * 4 + (fr & 3);
            const uint32_t ro = (uint32_t)row * (uint32_t)ldc;
            if constexpr (!CBF16) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                    quad_transpose(v, lane);
                    const skr::u32x4 o = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]),
                                          __float_as_uint(v[3])};
                    if (row < M) skr::st16<ST>(r, (ro + c0 + 16 * j + 4 * fc) * 4u, o);
                }
            } else {
#pragma unroll
                for (int j = 0; j < NJ; j += 2) {
                    uint32_t p[2][2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        float v[4] = {acc[i][j + h][0], acc[i][j + h][1], acc[i][j + h][2], acc[i][j + h][3]};
                        quad_transpose(v, lane);
                        p[h][0] = pack_bf16x2(v[0], v[1]);
                        p[h][1] = pack_bf16x2(v[2], v[3]);
                    }
                    // even column quads keep accumulator j (columns 4 fc .. + 7), odd ones j + 1
                    // (columns 4 (fc - 1) .. + 7): each sends the other accumulator's half 4 lanes across
                    const bool odd = fc & 1;
                    const uint32_t g0 = __shfl_xor(odd ? p[0][0] : p[1][0], 4, 64);
                    const uint32_t g1 = __shfl_xor(odd ? p[0][1] : p[1][1], 4, 64);
                    const skr::u32x4 o = odd ? skr::u32x4{g0, g1, p[1][0], p[1][1]}
                                             : skr::u32x4{p[0][0], p[0][1], g0, g1};
                    const int col = c0 + 16 * (j + (odd ? 1 : 0)) + 4 * (fc & ~1);
                    if (row < M) skr::st16<ST>(r, (ro + col) * 2u, o);
                }
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = 32 * wr + 16 * i + fq * 4 + e;
                if (row < M) {
                    const int64_t o = row * ldc + c0 + 16 * j + fr;
                    const float v = acc[i][j][e];   // (not bit_cast(acc[i][j][e]): see above)
                    if constexpr (CBF16) {
                        const __hip_bfloat16 b = skr::to_bf16(v);
                        if constexpr (ST == skr::ST_WT)   // global_store_short ... sc1
                            __hip_atomic_store((uint16_t*)Cv + o, __builtin_bit_cast(uint16_t, b), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                        else ((__hip_bfloat16*)Cv)[o] = b;
                    } else if constexpr (ST == skr::ST_WT) {   // relaxed agent-scope store = global_store_dword ... sc1
                        __hip_atomic_store((uint32_t*)Cv + o, __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    }
                    else ((float*)Cv)[o] = v;
                }
            }
}

// Workgroup `id` of a grouped launch: find its problem through the prefix
// sums `start` and run that tile.
template <int BN, int NS, int NW = 4, int ST = skr::ST_PLAIN, bool VEC = true>
__device__ __forceinline__ void group_tile(const GemmGroup& g, const int id, __hip_bfloat16* smem) {
    int q = 0;
#pragma unroll
    for (int i = 1; i < kMaxGroup; ++i) q += (i < g.n && id >= g.start[i]) ? 1 : 0;
    const GemmProblem& p = g.p[q];
    const TileIdx t = tile_idx(id - g.start[q], p.M, p.N, p.splits, BN);
    const int kslice = p.K / p.splits;
    glds_tile<BN, NS, false, NW, ST, VEC>((const __hip_bfloat16*)p.A + (int64_t)t.rb * skr::BM * p.lda, p.lda,
                                      (const __hip_bfloat16*)p.Bt, p.ldb, p.C + split_off(p, t), p.ldc, t.rows,
                                      t.nt * BN, (int64_t)t.split * kslice, kslice, smem);
}

// Host-side validation of one problem for 64-wide tiles (0: ok). M > 128:
// ceil(M / 128) row blocks, the last one partial (tile_idx: t.rows).
inline int check_problem64(const GemmProblem& p) {
    if (p.M < 1 || p.M > 8 * skr::BM || p.N % 64 != 0 || p.splits < 1 || p.K % p.splits != 0) return -2;
    if ((p.K / p.splits) % skr::BK != 0 || p.lda % 8 != 0 || p.ldb % 8 != 0) return -3;
    if (((uintptr_t)p.A | (uintptr_t)p.Bt) & 15) return -4;
    return 0;
}

}  // namespace
