// HyperLSTM modulation step (forward), one launch per time step:
//
//   vec   = hh_t @ P + q (+ the main bias in the shift block)       [B, 12 H]
//   g     = xh * vec_x + R * vec_h + vec_b                           [B, 4 H]
//   stats = per (row, gate, 32-unit tile): sum g, sum g^2
//
// Reference recurrence: /root/reference model.py:66-95 (static unroll);
// HyperLSTM semantics: sketch_rnn_amd/models/cells.py hyper_lstm_step.
//
// Why fused: the main cell's LayerNorm needs row statistics over all 2048
// units of each gate, so as its own kernel it spends one in-launch exchange
// between the workgroups of a row on them (~3 us per step). This kernel
// already owns every (row, unit) of the gate pre-activations it produces, so
// it emits per-tile partial sums (64 tiles per gate); the main cell
// (csrc/cell_fwd_body.h, MOD 3) sums them while loading -- one exchange per
// step fewer -- and reads the finished g (32 KB per row) instead of x-proj,
// the R slabs and the modulation vectors (144 KB per row).
// The saves the backward needs are written here too: the x and h blocks of
// vec (bf16, q folded in: the backward cell runs with a zero vec_bias) and
// the bf16 summed R.
//
// Tiling: workgroup (gate q, 32-unit tile u0) -> 4 x 64 = 256 workgroups of
// 384 threads. Wave w owns MFMA column tile w: k-block q + 4 (w / 2) (x, h,
// shift modulation of gate q), units u0 + 16 (w % 2) .. +15; its P
// fragments (8 k-steps, K = Hh = 256) live in VGPRs; hh (all rows, bf16) is
// staged once in LDS (XOR-swizzled rows). v_mfma_f32_16x16x32_bf16: lane l
// holds A[row l & 15][k 8 (l >> 4)..+7], B[k 8 (l >> 4)..+7][col l & 15];
// C: col l & 15, rows 4 (l >> 4) + i.
//
// (Round 4 measured an unfolded variant -- vec = bf16(hh W_z) W_a + q on two
// MFMA stages, W_z L2-resident instead of the 12.6 MB folded P -- at 12.9 vs
// 10.2 us per step, with a slower backward; profiles/r4/unfold_ab.txt.)
#include "common.h"
#include "store_policy.h"

namespace {

using namespace skr;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int HH = 256, NTH = 384, TU = 32;      // hyper units (K), threads, units per tile
constexpr int MAXB = 128;                        // rows (16-row MFMA tiles: NRT <= 8)

__device__ __forceinline__ int sw(int row, int chunk) { return row * HH + ((chunk ^ (row & 15)) << 3); }

__device__ __forceinline__ uint32_t pack_bf(float a, float b) {
    return (uint32_t)__bfloat16_as_ushort(__float2bfloat16(a)) |
           ((uint32_t)__bfloat16_as_ushort(__float2bfloat16(b)) << 16);
}

}  // namespace

// Decode-step inputs (sample/hyper_step.py, csrc/decode_step.hip): the main
// x-projection formed here from the sampled stroke x [B][5]:
// xh[b][n] = zp[b][n] + sum_k x[b][k] w5[k][n] (skr_bproj_fwd's order). Null
// members: the training sequence's input (precomputed xh).
struct ModDecode {
    int xh_bf16;                              // training: the precomputed xh is bf16 [B][4H] (not decode)
    const float* x5;
    const float* w5; int64_t ldw5;
    const float* zp; int64_t ldzp;
    int probe;                                // timing probe (skr_hyper_mod_set_probe; 0 = off), set by the host
    int st;                                   // write-through stores (csrc/store_policy.h), set by the host:
                                              // bit 0 the gate pre-activations g, bit 1 the saves (vec, rlp)
};

namespace {

// Row block z of a modulation tile (gate q, hidden units [TU tile, +TU); B >
// MAXB: the wide decode): rows r0 .. r0 + MAXB - 1.
// NRT: 16-row tiles staged and multiplied (rows up to 16 NRT; a B = 100 launch
// pays for 112 rows, not MAXB).
template <int NS, int NRT>
__device__ __forceinline__ void mod_block(ModDecode dec, const __hip_bfloat16* __restrict__ hh, int64_t ld_hh,
                                          const float* __restrict__ xh, const float* __restrict__ R, int64_t r_slab,
                                          __hip_bfloat16* __restrict__ vec, float* __restrict__ gout,
                                          __hip_bfloat16* __restrict__ rlp, float* __restrict__ stats, int B, int H,
                                          const int q, const int tile, const int z, const bf16x8 (&pf)[8],
                                          const float qv) {
    constexpr int MB = 16 * NRT;
    {
        const int r0 = z * MAXB;
        B = min(MAXB, B - r0);
        const int64_t G4 = (int64_t)r0 * 4 * H;
        if (hh) hh += (int64_t)r0 * ld_hh;
        if (dec.x5) {
            dec.x5 += (int64_t)r0 * 5;
            dec.zp += (int64_t)r0 * dec.ldzp;
        }
        if (xh) xh = dec.xh_bf16 ? (const float*)(const void*)((const __hip_bfloat16*)(const void*)xh + G4) : xh + G4;
        R += G4;
        gout += G4;
        if (rlp) rlp += G4;
        if (vec) vec += (int64_t)r0 * 12 * H;
        stats += (int64_t)r0 * 4 * (H / TU) * 2;
    }
    // (hh and the modulation vectors in one overlaid 64 KB buffer -- two
    // workgroups per CU, 130 VGPRs instead of 248 -- measured slower: the wide
    // decode's launch 64.2 vs 60.9 us, profiles/r6/dec2_kernels_bf16.txt)
    __shared__ __attribute__((aligned(16))) __hip_bfloat16 sA[MB * HH];     // <= 64 KB
    __shared__ __attribute__((aligned(16))) float sV[6][MB][16];            // <= 48 KB
    const int u0 = tile * TU, ntile = H / TU;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int G = 4 * H, NV = 12 * H;
    // ---- every global load up front (the P fragments: mod_tile): the
    // epilogue's x-projection and R slabs (thread -> rows rg, rg + 48, rg + 96;
    // units u0 + 4 ug .. +3), and hh for the LDS stage
    constexpr int RPT = (MB + NTH / 8 - 1) / (NTH / 8);      // rows per thread (<= 3)
    const int rg = tid >> 3, ug = tid & 7, ul = 4 * ug;
    f32x4 x4[RPT], r4[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int rr = min(rg + k * (NTH / 8), B - 1);
        const int64_t go = (int64_t)rr * G + q * H + u0 + ul;
        if (dec.x5 != nullptr) {
            const int col = q * H + u0 + ul;
            f32x4 v = *(const f32x4*)(dec.zp + rr * dec.ldzp + col);
#pragma unroll
            for (int k5 = 0; k5 < 5; ++k5) v += dec.x5[rr * 5 + k5] * *(const f32x4*)(dec.w5 + k5 * dec.ldw5 + col);
            x4[k] = v;
        } else if (dec.xh_bf16) {
            const uint2 u = *(const uint2*)((const __hip_bfloat16*)(const void*)xh + go);
            x4[k] = f32x4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                          __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
        } else {
            x4[k] = *(const f32x4*)(xh + go);
        }
        r4[k] = *(const f32x4*)(R + go);
#pragma unroll
        for (int sl = 1; sl < NS; ++sl) {
            const f32x4 t = *(const f32x4*)(R + sl * r_slab + go);
            r4[k] += t;
        }
    }
    if (dec.probe == 1) return;                 // (timing probe: dispatch + the P fragments only)
    constexpr int NPC = MB * (HH / 8), SPT = (NPC + NTH - 1) / NTH;     // 16-byte hh pieces per thread
    bf16x8 hv[SPT];
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int i = min(tid + k * NTH, NPC - 1), r = i / (HH / 8), c = i % (HH / 8);
        hv[k] = *(const bf16x8*)(hh + (int64_t)min(r, B - 1) * ld_hh + 8 * c);
    }
#pragma unroll
    for (int k = 0; k < SPT; ++k) {
        const int i = tid + k * NTH, r = i / (HH / 8), c = i % (HH / 8);
        if (i >= NPC) break;
        if (r >= B) hv[k] = bf16x8{};
        *(bf16x8*)(sA + sw(r, c)) = hv[k];
    }
    __syncthreads();
    if (dec.probe == 2) {                       // (timing probe: every load and the LDS stage, no MFMA / epilogue)
        float t = (float)pf[0][0] + __bfloat162float(sA[tid]);
#pragma unroll
        for (int k = 0; k < RPT; ++k) t += x4[k][0] + r4[k][0];
        if (t == 1.2345e-30f) gout[tid] = t;
        return;
    }
    f32x4 acc[NRT];
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            const bf16x8 a = *(const bf16x8*)(sA + sw(16 * rt + fr, 4 * ks + fq));
            acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pf[ks], acc[rt], 0, 0, 0);
        }
    if (dec.probe == 3) {                       // (timing probe: loads + MFMA, no vector stage / epilogue)
        float t = 0.f;
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) t += acc[rt][0];
#pragma unroll
        for (int k = 0; k < RPT; ++k) t += x4[k][0] + r4[k][0];
        if (t == 1.2345e-30f) gout[tid] = t;
        return;
    }
    // modulation vectors (+ q) -> bf16 -> LDS: the epilogue needs all three
    // blocks of a unit in one thread. The bf16-rounded value is what the
    // backward will read, so g is formed from it too.
#pragma unroll
    for (int rt = 0; rt < NRT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            sV[w][16 * rt + 4 * fq + i][fr] = __bfloat162float(__float2bfloat16(acc[rt][i] + qv));
    __syncthreads();
    // ---- epilogue (no loads left): 8 threads per row (lanes 8k..8k+7)
    const int ch = ul >> 4, cu = ul & 15;          // column tile half, column inside it
    // (write-through arms, dec.st: buffer descriptors of this row block's outputs)
    const __amdgpu_buffer_rsrc_t rg_ = skr::rsrc(gout, (int64_t)B * G * 4), rr_ = skr::rsrc(rlp, (int64_t)B * G * 2),
                                 rv_ = skr::rsrc(vec, (int64_t)B * NV * 2);
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int r = rg + k * (NTH / 8);
        if (r >= ((B + 7) & ~7)) break;            // uniform over each 8-lane row group and each wave
        const bool on = r < B;
        const int rr = on ? r : B - 1;
        float g[4], s1 = 0.f, s2 = 0.f;
        float vx[4], vh[4], vb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            vx[i] = sV[0 + ch][rr][cu + i];
            vh[i] = sV[2 + ch][rr][cu + i];
            vb[i] = sV[4 + ch][rr][cu + i];
            g[i] = x4[k][i] * vx[i] + r4[k][i] * vh[i] + vb[i];
            s1 += g[i];
            s2 += g[i] * g[i];
        }
        s1 += __shfl_xor(s1, 1, 64);
        s2 += __shfl_xor(s2, 1, 64);
        s1 += __shfl_xor(s1, 2, 64);
        s2 += __shfl_xor(s2, 2, 64);
        s1 += __shfl_xor(s1, 4, 64);
        s2 += __shfl_xor(s2, 4, 64);
        if (on) {
            const int64_t go = (int64_t)rr * G + q * H + u0 + ul;
            const int64_t vo = (int64_t)rr * NV + u0 + ul;
            const u32x2 rl = {pack_bf(r4[k][0], r4[k][1]), pack_bf(r4[k][2], r4[k][3])};
            const u32x2 px = {pack_bf(vx[0], vx[1]), pack_bf(vx[2], vx[3])}, ph = {pack_bf(vh[0], vh[1]), pack_bf(vh[2], vh[3])};
            if (dec.st & 1)
                skr::st16<skr::ST_WT>(rg_, (uint32_t)go * 4u, skr::u32x4{__float_as_uint(g[0]), __float_as_uint(g[1]),
                                                                         __float_as_uint(g[2]), __float_as_uint(g[3])});
            else *(f32x4*)(gout + go) = f32x4{g[0], g[1], g[2], g[3]};
            if (dec.st & 2) {
                if (rlp) skr::st8<skr::ST_WT>(rr_, (uint32_t)go * 2u, rl[0], rl[1]);
                if (vec) {
                    skr::st8<skr::ST_WT>(rv_, (uint32_t)(vo + q * H) * 2u, px[0], px[1]);
                    skr::st8<skr::ST_WT>(rv_, (uint32_t)(vo + (4 + q) * H) * 2u, ph[0], ph[1]);
                }
            } else {
                if (rlp) *(u32x2*)(rlp + go) = rl;
                if (vec) {   // (null at inference)
                    *(u32x2*)(vec + vo + q * H) = px;
                    *(u32x2*)(vec + vo + (4 + q) * H) = ph;
                }
            }
            // (the shift block 8..11 is not stored: the backward reads only
            // the x and h modulations -- d(shift) = dg needs no saved value)
            if (ug == 0) {
                const int64_t so = (((int64_t)rr * 4 + q) * ntile + tile) * 2;
                stats[so] = s1;
                stats[so + 1] = s2;
            }
        }
    }
}

// One modulation tile: gate q, hidden units [TU tile, +TU), row blocks z0,
// z0 + zs, ... of B rows (the P fragments loaded once for all of them).
template <int NS, int NRT>
__device__ __forceinline__ void mod_tile(ModDecode dec, const __hip_bfloat16* __restrict__ hh, int64_t ld_hh,
                                         const __hip_bfloat16* __restrict__ PlT,   // [12H][HH]
                                         const float* __restrict__ qb,             // [12H]
                                         const float* __restrict__ xh,             // [B][4H]
                                         const float* __restrict__ R, int64_t r_slab,   // [NS][B][4H]
                                         __hip_bfloat16* __restrict__ vec,          // [B][12H]
                                         float* __restrict__ gout,                  // [B][4H]
                                         __hip_bfloat16* __restrict__ rlp,          // [B][4H] or null
                                         float* __restrict__ stats,                 // [B][4][H/TU][2]
                                         int B, int H, const int q, const int tile, const int z0, const int zs) {
    const int u0 = tile * TU;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int vcol = (q + 4 * (w >> 1)) * H + u0 + 16 * (w & 1);   // first modulation column of tile w
    bf16x8 pf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) pf[ks] = *(const bf16x8*)(PlT + (int64_t)(vcol + fr) * HH + 32 * ks + 8 * fq);
    const float qv = qb[vcol + fr];
    const int nblk = (B + MAXB - 1) / MAXB;
    // (consecutive blocks reuse the LDS: the next block's hh stage is written
    // after this block's MFMAs -- every wave passed this block's second
    // barrier -- and its vectors after the next block's first barrier)
    for (int z = z0; z < nblk; z += zs)
        mod_block<NS, NRT>(dec, hh, ld_hh, xh, R, r_slab, vec, gout, rlp, stats, B, H, q, tile, z, pf, qv);
}

template <int NS, int NRT>
__global__ __launch_bounds__(NTH) void hyper_mod_fwd(ModDecode dec, const __hip_bfloat16* __restrict__ hh, int64_t ld_hh,
                                                     const __hip_bfloat16* __restrict__ PlT, const float* __restrict__ qb,
                                                     const float* __restrict__ xh, const float* __restrict__ R,
                                                     int64_t r_slab, __hip_bfloat16* __restrict__ vec,
                                                     float* __restrict__ gout, __hip_bfloat16* __restrict__ rlp,
                                                     float* __restrict__ stats, int B, int H) {
    if (dec.probe == 4) return;   // (timing probe: dispatch only)
    mod_tile<NS, NRT>(dec, hh, ld_hh, PlT, qb, xh, R, r_slab, vec, gout, rlp, stats, B, H, blockIdx.y, blockIdx.x,
                      blockIdx.z, gridDim.z);
}

}  // namespace

static int g_hm_zgrid = 0;   // row blocks in parallel (0: all); skr_hyper_mod_set_zgrid
static int g_hm_probe = 0;   // timing probe of skr_hyper_mod_fwd (the outputs are WRONG while set)

// Timing probes (scripts/micro/hm_probe.py): 0 off, 1 each row block returns
// at once (dispatch + P fragment loads), 2 after every load and the hh LDS
// stage, 3 after the MFMAs (no vector stage, epilogue or stores), 4 every
// workgroup returns at entry (dispatch only). Returns the previous setting.
SKR_API int skr_hyper_mod_set_probe(int p) {
    const int prev = g_hm_probe;
    if (p >= 0) g_hm_probe = p;
    return prev;
}

// A/B hook: parallel row blocks of the wide (B > 128) launches; 0 = one
// workgroup per row block. Returns the previous setting.
SKR_API int skr_hyper_mod_set_zgrid(int zg) {
    const int prev = g_hm_zgrid;
    if (zg >= 0) g_hm_zgrid = zg;
    return prev;
}

// hh [B][Hh] bf16 rows (stride ld_hh), PlT [12H][Hh] bf16, qb [12H] fp32
// (q, with the main bias added to blocks 8..11), xh [B][4H] fp32, R = sum of
// nslab fp32 slabs [B][4H] (stride r_slab), outputs vec [B][12H] bf16 (blocks
// 0..7 written; null at inference), g [B][4H] fp32, rlp [B][4H] bf16 (or
// null), stats [B][4][H/32][2] fp32. dec: decode-step inputs (ModDecode) or
// null. B > 128: 128-row blocks over gridDim.z (the last one partial).
SKR_API int skr_hyper_mod_fwd(const void* hh, int64_t ld_hh, const void* PlT, const float* qb, const float* xh,
                              const float* R, int64_t r_slab, int nslab, void* vec, float* g, void* rlp,
                              float* stats, int B, int H, int Hh, const ModDecode* dec, hipStream_t s) {
    ModDecode dz = dec ? *dec : ModDecode{};
    dz.probe = g_hm_probe;
    dz.st = (skr_store_policy_of(skr::SC_STEP) == skr::ST_WT ? 1 : 0) | (skr_store_policy_of(skr::SC_SAVE) == skr::ST_WT ? 2 : 0);
    if (dz.x5 && (((uintptr_t)dz.w5 | (uintptr_t)dz.zp) & 15 || dz.ldw5 % 4 || dz.ldzp % 4)) return -4;
    if ((dz.x5 == nullptr && xh == nullptr) || hh == nullptr) return -3;
    if (B <= 0) return 0;
    if (B > 8 * MAXB || Hh != HH || H % TU != 0) return -2;
    if (((uintptr_t)hh | (uintptr_t)PlT | (uintptr_t)xh | (uintptr_t)R | (uintptr_t)vec | (uintptr_t)g |
         (uintptr_t)rlp) & 15 || (ld_hh % 8) || (r_slab % 4))
        return -4;
    // row blocks: gridDim.z of them in parallel, each workgroup walking
    // blocks z, z + gridDim.z, ... with its P fragments loaded once
    const int nblk = (B + MAXB - 1) / MAXB;
    const dim3 grid(H / TU, 4, g_hm_zgrid > 0 ? (nblk < g_hm_zgrid ? nblk : g_hm_zgrid) : nblk);
    const auto* a = (const __hip_bfloat16*)hh;
    const auto* p = (const __hip_bfloat16*)PlT;
    auto* v = (__hip_bfloat16*)vec;
    auto* rl = (__hip_bfloat16*)rlp;
    const int nrt = B <= 32 ? 2 : B <= 64 ? 4 : B <= 112 ? 7 : 8;
    if (nslab != 1 && nslab != 2 && nslab != 4) return -3;
#define SKR_HM(NS_, NRT_) \
    hipLaunchKernelGGL((hyper_mod_fwd<NS_, NRT_>), grid, dim3(NTH), 0, s, dz, a, ld_hh, p, qb, xh, R, r_slab, v, g, rl, stats, B, H)
#define SKR_HM_NS(NRT_) \
    do { if (nslab == 1) SKR_HM(1, NRT_); else if (nslab == 2) SKR_HM(2, NRT_); else SKR_HM(4, NRT_); } while (0)
    switch (nrt) {
        case 2: SKR_HM_NS(2); break;
        case 4: SKR_HM_NS(4); break;
        case 7: SKR_HM_NS(7); break;
        default: SKR_HM_NS(8); break;
    }
#undef SKR_HM_NS
#undef SKR_HM
    return SKR_CHECK_LAUNCH();
}
