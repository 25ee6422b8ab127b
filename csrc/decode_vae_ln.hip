// Fused whole-sketch decoder for the VAE's LayerNorm-LSTM decoders
// (dec_model "layer_norm"; models/cells.py ln_lstm_pointwise as
// SketchVAE.decode_step calls it). Roles, geometry, step ranges, prefixes and
// the head are those of csrc/decode_vae.hip (the head, stage() and frag() are
// shared: csrc/decode_head.h); what is new is the layer step.
//
// Step t of row b, layer workgroup wu (units u0 .. u0 + 15 of every gate):
//   g[q][u] = h(t-1) . W_h[:, qH+u]  (bf16 MFMA, fp32 accumulation)
//           + x(t) . W_x[:5, qH+u] + zp[b][qH+u]           (fp32; no bias)
//   gn      = (g - mean_q) * rsqrt(var_q + 1e-3) * ln_gamma + ln_beta, the
//             mean and biased variance over the H columns of gate q
//   c'      = c * sigmoid(gn_f + forget_bias) + sigmoid(gn_i) * tanh(gn_j)
//   h'      = tanh(LN(c'; lnc_gamma, lnc_beta)) * sigmoid(gn_o)
// The carried c is the un-normalised c' (fp32, VGPRs); h' goes to hbuf[t+1]
// as bf16.
//
// Statistics exchange (direct form). A workgroup holds 16 of the H columns of
// each gate, so both layer norms need the other H/16 - 1 workgroups of the
// row block. Per row (and gate) a workgroup reduces its 16 values to
// (mean_k, M2_k = sum (v - mean_k)^2) with an xor butterfly over `lane & 15`
// (every lane ends with the same bits), stores the pair with sc1 stores into
// its own slot and publishes an epoch (handoff.h protocol, unchanged). After
// waiting for all H/16 epochs, a lane reads the H/16 pairs of one (row, gate)
// with sc1 loads and combines them IN WORKGROUP-INDEX ORDER (equal counts:
//   mean = sum_k mean_k / NW,  M2 = sum_k M2_k + 16 * sum_k (mean_k - mean)^2),
// so the result does not depend on arrival order, on the launch split or on
// which workgroup computes it: every workgroup derives bit-identical
// statistics. No E[x^2] - E[x]^2 cancellation occurs anywhere.
//
// Slot reuse. The slots are indexed by step parity, which is more than is
// needed: a workgroup stores step t+1's partials only after its tile's waves
// have waited for ALL h epochs t+1 of the row block (the wait in front of the
// MFMAs), and a workgroup publishes h epoch t+1 only after its loads of step
// t's partials have returned (the h it stores depends on them, and publish()
// drains vmcnt). So every reader of step t's slots is done before any writer
// of step t+1's; parity adds a second step of slack for free.
//
// Flag words per row block (kLnFlagStride = 128, zeroed per launch by
// zero_flags): [0, NW) h epochs | NW head | [64, 64+NW) gate-statistics
// epochs | [96, 96+NW) cell-statistics epochs, NW = H/16 <= 32.
//
// Rows past B of a partial row block are clamped duplicates of row B - 1, as
// in the plain kernel: their statistics go to their own (in-range) slot rows,
// no real row reads them, and nothing of theirs is stored to hbuf / cT.
#include <algorithm>

#include "decode_head.h"

struct DecVaeLnArgs {
    int N, B, H, mtw, nrb, M, nout, noutp, greedy;
    int row0;                            // global index of row 0 (sampler hash: batches split over launches)
    int t0, t1;                          // global step range of this launch
    float temp, forget_bias;
    const __hip_bfloat16* WT;            // [4H][H] W_h^T
    const float* Wx;                     // [5][4H] stroke rows of W_x (fp32)
    const float* zp;                     // [B][4H] zc @ W_x[5:] (zero rows without a z input)
    const float* ln_g;                   // [4H] gate layer norm
    const float* ln_b;                   // [4H]
    const float* lnc_g;                  // [H] cell layer norm
    const float* lnc_b;                  // [H]
    const float* c0;                     // [B][H] cell state entering step t0
    float* cT;                           // [B][H] cell state after step t1 - 1 (may alias c0)
    __hip_bfloat16* hbuf;                // [N+1][B][H] h entering step t; hbuf[0] = h0 (host)
    const __hip_bfloat16* WoT;           // [noutp][H] head weights^T (rows >= nout zero)
    const float* bo;                     // [nout]
    float* xin;                          // [N+1][B][8] fed inputs (x(0) and the prefixes from the host)
    float* out;                          // [B][N][5] strokes
    int* done;                           // [B] finished state: read at t0, written after t1 - 1
    const int* nforced;                  // [B] leading strokes taken from xin, or null (0)
    const float* temps;                  // [B] per-row temperature in place of temp, or null
    float* zout;                         // [N][B][nout] head outputs, or null
    float* gstat;                        // [2][nrb][H/16][16*mtw][4][2] gate (mean, M2) partials
    float* cstat;                        // [2][nrb][H/16][16*mtw][2] cell (mean, M2) partials
    const int64_t* seed;
    uint32_t* flags;                     // [nrb][kLnFlagStride] epochs (zeroed per launch)
    int* err;
};

namespace {

using namespace skr;

constexpr int kLnFlagStride = 128;
constexpr int kGateFlag = 64, kCellFlag = 96;
constexpr float kLnEps = 1e-3f;

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void st_sc1_f32x2(__amdgpu_buffer_rsrc_t r, uint32_t off, float x, float y) {
    __builtin_amdgcn_raw_buffer_store_b64(u32x2{__builtin_bit_cast(uint32_t, x), __builtin_bit_cast(uint32_t, y)}, r,
                                          off, 0, kSc1);
}
// Two 4-byte loads, not __builtin_amdgcn_raw_buffer_load_b64: hipcc of ROCm
// 7.x compiles that builtin to ONE buffer_load_dword whose value fills both
// elements (seen in the assembly); the b64 store and the b32 / b128 loads are
// compiled as written.
__device__ __forceinline__ void ld_sc1_f32x2(__amdgpu_buffer_rsrc_t r, uint32_t off, float& x, float& y) {
    x = ld_sc1_f32(r, off);
    y = ld_sc1_f32(r, off + 4);
}

// sum over the 16 lanes that share lane >> 4; xor butterfly: every lane of
// the group ends with the same bits
__device__ __forceinline__ float sum16(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// NW (mean_k, M2_k) pairs of 16 values each, `stride` bytes apart from `off`,
// combined in k order -> mean and rsqrt(var + eps) over the 16 * NW values
template <int NW>
__device__ __forceinline__ void combine(__amdgpu_buffer_rsrc_t r, uint32_t off, uint32_t stride, float& mean,
                                        float& rstd) {
    float m[NW], q[NW];
#pragma unroll
    for (int k = 0; k < NW; ++k) ld_sc1_f32x2(r, off + (uint32_t)k * stride, m[k], q[k]);
    float sm = 0.f, sq = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        sm += m[k];
        sq += q[k];
    }
    mean = sm * (1.0f / NW);
    float sd = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const float d = m[k] - mean;
        sd += d * d;
    }
    rstd = rsqrtf((sq + 16.0f * sd) * (1.0f / (16 * NW)) + kLnEps);
}

// ---------------------------------------------------------------------------------
// the LayerNorm-LSTM layer's unit block
// ---------------------------------------------------------------------------------
template <int H, int MTW>
__device__ void layer_body(const DecVaeLnArgs& a, int rb, int wu, unsigned char* smem) {
    constexpr int K = H, KS = 8 / MTW, KP = K / KS, NKS = KP / 32, NW = H / U, RB = 16 * MTW;
    __hip_bfloat16* Ws = (__hip_bfloat16*)smem;                        // [64][K]
    f32x4* part = (f32x4*)(smem + 64 * K * 2);                         // [KS][MTW][4][64]
    __hip_bfloat16* hx = (__hip_bfloat16*)(part + KS * MTW * 4 * 64);  // [MTW][16][16]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int mt = w % MTW, kp = w / MTW;
    const int fr = lane & 15, fq = lane >> 4;
    const int B = a.B, N = a.N;
    const int u0 = wu * U;
    const int row_t0 = rb * RB + mt * 16;       // first row of this wave's tile
    const bool tile_on = row_t0 < B;

    stage<true>(Ws, a.WT, 64, K, H, u0);
    __syncthreads();

    uint32_t* fl = a.flags + (int64_t)rb * kLnFlagStride;
    uint32_t* my_flags = fl;
    const uint32_t* head_flag = fl + NW;
    uint32_t* gate_flags = fl + kGateFlag;
    uint32_t* cell_flags = fl + kCellFlag;
    const __amdgpu_buffer_rsrc_t r_h = rsrc(a.hbuf, (int64_t)(N + 1) * B * H * 2);
    const __amdgpu_buffer_rsrc_t r_x = rsrc(a.xin, (int64_t)(N + 1) * B * kXLd * 4);
    // statistics slots of one parity and row block: [NW][RB rows][4][2] and [NW][RB rows][2]
    constexpr uint32_t kGSlot = RB * 4 * 2 * 4, kCSlot = RB * 2 * 4;   // bytes per workgroup
    const int64_t gpar = (int64_t)a.nrb * NW * kGSlot, cpar = (int64_t)a.nrb * NW * kCSlot;
    const __amdgpu_buffer_rsrc_t r_g = rsrc(a.gstat, 2 * gpar);
    const __amdgpu_buffer_rsrc_t r_c = rsrc(a.cstat, 2 * cpar);

    // epilogue lanes: K-slice-0 waves; lane holds rows row_t0 + 4fq + e, unit u0 + fr
    const bool epi = kp == 0 && tile_on;
    const int u = u0 + fr;
    int brow[4];
    bool bon[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int r = row_t0 + 4 * fq + e;
        bon[e] = epi && r < B;
        brow[e] = min(r, B - 1);
    }
    float c[4], zp[4][4], wx[5][4], lg[4], lb[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        c[e] = epi ? a.c0[(int64_t)brow[e] * H + u] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) zp[e][q] = epi ? a.zp[(int64_t)brow[e] * 4 * H + q * H + u] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        lg[q] = a.ln_g[q * H + u];
        lb[q] = a.ln_b[q * H + u];
#pragma unroll
        for (int i = 0; i < 5; ++i) wx[i][q] = a.Wx[i * 4 * H + q * H + u];
    }
    const float cg = a.lnc_g[u], cb = a.lnc_b[u];
    // x(t) of row b comes from the head's step t - 1 iff t > nforced[b]: the
    // tile waits for the head from the first such step of any of its rows
    int min_nf = 0;
    if (a.nforced != nullptr && tile_on) {
        min_nf = N;
        for (int r = row_t0; r < min(row_t0 + 16, B); ++r) min_nf = min(min_nf, a.nforced[r]);
    }
    const int arow = min(row_t0 + fr, B - 1);   // A-fragment row of this lane (clamped)
    // exchange roles of a lane: it combines gate (fr & 3) of tile row
    // 4fq + (fr >> 2), and the cell statistics of tile row 4fq + (fr & 3)
    const int trow = mt * 16 + 4 * fq;          // first of this lane's 4 rows within the row block
    const uint32_t g_my = (uint32_t)((trow * 4 + fr) * 8);          // [row 4fq + (fr >> 2)][gate fr & 3]
    const uint32_t c_my = (uint32_t)((trow + (fr & 3)) * 8);
    bool ok = true;

    for (int t = a.t0; t < a.t1; ++t) {
        const uint32_t g_base = (uint32_t)((t & 1) * gpar + (int64_t)rb * NW * kGSlot);
        const uint32_t c_base = (uint32_t)((t & 1) * cpar + (int64_t)rb * NW * kCSlot);
        f32x4 acc[4] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f},
                        f32x4{0.f, 0.f, 0.f, 0.f}};
        if (tile_on) {
            const int k0 = kp * KP;
            if (t > a.t0) ok = ok && wait_flags(my_flags, NW, (uint32_t)t, a.err);
            const uint32_t base = (uint32_t)(((int64_t)t * B + arow) * H * 2);
            bf16x8 af[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) af[ks] = ld_sc1(r_h, base + (uint32_t)((k0 + ks * 32 + fq * 8) * 2));
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const int chunk = (k0 + ks * 32) / 8 + fq;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], frag(Ws, q * 16 + fr, K, chunk), acc[q],
                                                                     0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) part[((kp * MTW + mt) * 4 + q) * 64 + lane] = acc[q];
        }
        __syncthreads();
        float g[4][4];   // [row e][gate q]
        if (epi) {
            // fed input x(t): drawn by the head at step t - 1 of this launch
            if (t > a.t0 && t > min_nf) ok = ok && wait_flags(head_flag, 1, (uint32_t)t, a.err);
            float xv[4][5];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 5; ++i)
                    xv[e][i] = ld_sc1_f32(r_x, (uint32_t)((((int64_t)t * B + brow[e]) * kXLd + i) * 4));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 s = part[(mt * 4 + q) * 64 + lane];
#pragma unroll
                for (int p = 1; p < KS; ++p) s += part[((p * MTW + mt) * 4 + q) * 64 + lane];
                acc[q] = s;
            }
            // this lane's pair to publish: (row e, gate q) with 4e + q == fr
            float pm = 0.f, pq = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v = acc[q][e] + zp[e][q];
#pragma unroll
                    for (int i = 0; i < 5; ++i) v += xv[e][i] * wx[i][q];
                    g[e][q] = v;
                    const float m = sum16(v) * (1.0f / 16);
                    const float d = v - m;
                    const float m2 = sum16(d * d);
                    if (fr == 4 * e + q) {
                        pm = m;
                        pq = m2;
                    }
                }
            st_sc1_f32x2(r_g, g_base + (uint32_t)wu * kGSlot + g_my, pm, pq);
        }
        publish(gate_flags + wu, (uint32_t)(t + 1));
        if (epi) {
            ok = ok && wait_flags(gate_flags, NW, (uint32_t)(t + 1), a.err);
            float mean, rstd;
            combine<NW>(r_g, g_base + g_my, kGSlot, mean, rstd);
            float pm = 0.f, pq = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float gn[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int src = (lane & 48) + 4 * e + q;
                    const float mu = __shfl(mean, src), rs = __shfl(rstd, src);
                    gn[q] = (g[e][q] - mu) * rs * lg[q] + lb[q];
                }
                const float ig = sigmoidf_(gn[0]), tj = tanhf(gn[1]), fg = sigmoidf_(gn[2] + a.forget_bias);
                g[e][3] = sigmoidf_(gn[3]);     // the output gate, kept for h
                c[e] = c[e] * fg + ig * tj;
                const float m = sum16(c[e]) * (1.0f / 16);
                const float d = c[e] - m;
                const float m2 = sum16(d * d);
                if ((fr & 3) == e) {
                    pm = m;
                    pq = m2;
                }
            }
            if (fr < 4) st_sc1_f32x2(r_c, c_base + (uint32_t)wu * kCSlot + c_my, pm, pq);
        }
        publish(cell_flags + wu, (uint32_t)(t + 1));
        if (epi) {
            ok = ok && wait_flags(cell_flags, NW, (uint32_t)(t + 1), a.err);
            float mean, rstd;
            combine<NW>(r_c, c_base + c_my, kCSlot, mean, rstd);
            float hn[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int src = (lane & 48) + e;
                const float mu = __shfl(mean, src), rs = __shfl(rstd, src);
                hn[e] = tanhf(cg * (c[e] - mu) * rs + cb) * g[e][3];
            }
            // h -> hbuf[t+1]: transposed through LDS so each store is 16
            // contiguous bytes (8 units of one row)
            __hip_bfloat16* hw = hx + mt * 256;
#pragma unroll
            for (int e = 0; e < 4; ++e) hw[(4 * fq + e) * 16 + fr] = to_bf16(hn[e]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane < 32) {
                const int r = lane >> 1, hf = lane & 1;
                if (row_t0 + r < B) {
                    const u32x4 v = *(const u32x4*)(hw + r * 16 + hf * 8);
                    const int64_t off = ((int64_t)(t + 1) * B + row_t0 + r) * H + u0 + hf * 8;
                    st_sc1(r_h, (uint32_t)(off * 2), v);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        publish(my_flags + wu, (uint32_t)(t + 1));
    }
    if (epi) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (bon[e]) a.cT[(int64_t)brow[e] * H + u] = c[e];
    }
    (void)ok;
}

template <int H, int MTW>
__global__ __launch_bounds__(NTHR) void decode_vae_ln_kernel(const DecVaeLnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int per = H / U + 1;
    const int rb = blockIdx.x / per, role = blockIdx.x - rb * per;
    if (role == H / U) {
        head_body<H, MTW, kLnFlagStride>(a, rb, smem);
    } else {
        layer_body<H, MTW>(a, rb, role, smem);
    }
}

inline size_t layer_lds(int H, int mtw) {
    return (size_t)64 * H * 2 + (size_t)(8 / mtw) * mtw * 4 * 64 * 16 + (size_t)mtw * 256 * 2;
}
constexpr size_t kMaxLds = 160 * 1024;

template <int H, int MTW>
int launch(const DecVaeLnArgs& a, hipStream_t s) {
    const size_t lds = std::max(layer_lds(H, MTW), head_lds(H, a.noutp, MTW));
    if (lds > kMaxLds) return -2;
    const int grid = a.nrb * (H / U + 1);
    auto kern = decode_vae_ln_kernel<H, MTW>;
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds) !=
            hipSuccess)
            return -9;
        attr = true;
    }
    if (!grid_fits((const void*)kern, NTHR, lds, grid)) return -8;
    const int nflags = a.nrb * kLnFlagStride;
    hipLaunchKernelGGL(zero_flags, dim3((nflags + 255) / 256), dim3(256), 0, s, a.flags, nflags);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NTHR), lds, s, a);
    return SKR_CHECK_LAUNCH();
}

}  // namespace

// Steps [t0, t1) of B sketches. Rows per row block: 16 * mtw (mtw 1 or 2).
// Eligible: H 256 with 1..32 mixtures, H 512 with 1..20 (the head's LDS).
// Returns 0 on success, < 0 on a rejected call (-2 geometry, -4 nrb, -6
// missing buffers, -8 grid not co-resident, -11 offsets past 32 bits).
SKR_API int skr_decode_vae_ln(const DecVaeLnArgs* a, hipStream_t s) {
    if (a->N <= 0 || a->B <= 0 || a->t0 == a->t1) return 0;
    if (a->t0 < 0 || a->t1 > a->N || a->t0 > a->t1) return -2;
    if ((a->H != 256 && a->H != 512) || (a->mtw != 1 && a->mtw != 2)) return -2;
    if (a->M < 1 || a->M > (a->H == 256 ? 32 : 20) || a->nout != 3 + 6 * a->M ||
        a->noutp != (a->nout + 15) / 16 * 16)
        return -2;
    if (a->nrb != (a->B + 16 * a->mtw - 1) / (16 * a->mtw)) return -4;
    if (a->WT == nullptr || a->Wx == nullptr || a->zp == nullptr || a->ln_g == nullptr || a->ln_b == nullptr ||
        a->lnc_g == nullptr || a->lnc_b == nullptr || a->c0 == nullptr || a->cT == nullptr || a->hbuf == nullptr ||
        a->WoT == nullptr || a->bo == nullptr || a->xin == nullptr || a->out == nullptr || a->done == nullptr ||
        a->gstat == nullptr || a->cstat == nullptr || a->seed == nullptr || a->flags == nullptr || a->err == nullptr)
        return -6;
    if ((int64_t)(a->N + 1) * a->B * a->H * 2 > 0x7fffffffLL || (int64_t)(a->N + 1) * a->B * kXLd * 4 > 0x7fffffffLL)
        return -11;
    if (a->H == 256) return a->mtw == 1 ? launch<256, 1>(*a, s) : launch<256, 2>(*a, s);
    return a->mtw == 1 ? launch<512, 1>(*a, s) : launch<512, 2>(*a, s);
}

SKR_API int skr_decode_vae_ln_args_size() { return (int)sizeof(DecVaeLnArgs); }
