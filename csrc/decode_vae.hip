// Fused whole-sketch decoder for the VAE's plain LSTM decoders (SURVEY K13;
// the sketch-rnn sampling loop around SketchVAE.decode_step): one launch
// generates steps [t0, t1) of B sketches -- per step the LSTM layer, the MDN
// head and the sampler -- with no host round trip and no kernel boundary
// between strokes. Structure and hand-offs follow csrc/decode_ref.hip.
//
// Roles (per row block of RB = 16*MTW sketches, H/16 + 1 workgroups):
//   layer, unit block wu (16 hidden units = 64 gate columns): keeps its
//     columns of W_h in LDS for the whole launch and c in VGPRs; bf16 MFMA
//     (v_mfma_f32_16x16x32_bf16) over K = H split across 8/MTW wave groups,
//     fp32 cell. The epilogue adds x(t) @ W_x[:5] and the per-row bias
//     zb[b] = zc[b] @ W_x[5:] + bias (host, once per run) in fp32. Gate order
//     i, j, f, o (models/cells.py lstm_pointwise). The VAE has no eoc state
//     hold: the carried h is the output h, one buffer (hbuf[t+1]) serves the
//     next step and the head.
//   head: keeps W_out^T (padded to a multiple of 16 rows) in LDS, computes
//     z = h(t) @ W_out + b for its RB rows with MFMA into LDS, then one wave
//     per row draws the stroke (csrc/mdn_sample.h, mode 1, bit-identical with
//     the stand-alone sampler kernel) and writes it as the next input x(t+1).
// Critical path per stroke: head(t-1) -> layer epilogue (t) -> head (t); the
// layer's recurrent MFMAs of step t only need h(t-1) and run while the head
// is still sampling x(t).
//
// Step ranges: the buffers cover the whole sketch and every index, flag
// epoch and sampler key uses the global step t. A launch with t0 > 0 reads c
// from `c0` (the previous launch's `cT`; the two may alias), h from hbuf[t0],
// x from xin[t0] and the finished state from done[b]: all written by the
// previous launch, so its first step needs no wait, and [0, a) then [a, b)
// computes the same bits as [0, b).
//
// Per-row prefix: the first nforced[b] strokes of row b are taken from xin
// (x(1..nforced) from the host): for t < nforced[b] the head leaves x(t+1)
// alone, emits out[b][t] = xin[t+1][b] and takes the finished state from that
// row's pen. Teacher forcing is nforced[b] = N. Finished rows emit
// end-of-sketch padding [0,0,0,0,1] while the recurrence keeps running, as
// GraphDecoder + csrc/sampler.hip do.
//
// stage(), frag() and the head role live in csrc/decode_head.h, shared with
// the layer_norm decoder (csrc/decode_vae_ln.hip).
#include <algorithm>

#include "decode_head.h"

struct DecVaeArgs {
    int N, B, H, mtw, nrb, M, nout, noutp, greedy;
    int row0;                            // global index of row 0 (sampler hash: batches split over launches)
    int t0, t1;                          // global step range of this launch
    float temp, forget_bias;
    const __hip_bfloat16* WT;            // [4H][H] W_h^T
    const float* Wx;                     // [5][4H] stroke rows of W_x (fp32)
    const float* zb;                     // [B][4H] per-row bias: zc @ W_x[5:] + bias
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
    const int64_t* seed;
    uint32_t* flags;                     // [nrb][kFlagStride] epochs (zeroed per launch)
    int* err;
};

namespace {

using namespace skr;

constexpr int kFlagStride = 64;  // flag words per row block: [layer (H/16) | head]

// ---------------------------------------------------------------------------------
// the LSTM layer's unit block
// ---------------------------------------------------------------------------------
template <int H, int MTW>
__device__ void layer_body(const DecVaeArgs& a, int rb, int wu, unsigned char* smem) {
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

    uint32_t* fl = a.flags + (int64_t)rb * kFlagStride;
    uint32_t* my_flags = fl;
    const uint32_t* head_flag = fl + NW;
    const __amdgpu_buffer_rsrc_t r_h = rsrc(a.hbuf, (int64_t)(N + 1) * B * H * 2);
    const __amdgpu_buffer_rsrc_t r_x = rsrc(a.xin, (int64_t)(N + 1) * B * kXLd * 4);

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
    float c[4], zb[4][4], wx[5][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        c[e] = epi ? a.c0[(int64_t)brow[e] * H + u] : 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) zb[e][q] = epi ? a.zb[(int64_t)brow[e] * 4 * H + q * H + u] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 5; ++i) wx[i][q] = a.Wx[i * 4 * H + q * H + u];
    // x(t) of row b comes from the head's step t - 1 iff t > nforced[b]: the
    // tile waits for the head from the first such step of any of its rows
    int min_nf = 0;
    if (a.nforced != nullptr && tile_on) {
        min_nf = N;
        for (int r = row_t0; r < min(row_t0 + 16, B); ++r) min_nf = min(min_nf, a.nforced[r]);
    }
    const int arow = min(row_t0 + fr, B - 1);   // A-fragment row of this lane (clamped)
    bool ok = true;

    for (int t = a.t0; t < a.t1; ++t) {
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
            float hn[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float g[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v = acc[q][e] + zb[e][q];
#pragma unroll
                    for (int i = 0; i < 5; ++i) v += xv[e][i] * wx[i][q];
                    g[q] = v;
                }
                const float ig = sigmoidf_(g[0]), tj = tanhf(g[1]), fg = sigmoidf_(g[2] + a.forget_bias);
                const float og = sigmoidf_(g[3]);
                c[e] = c[e] * fg + ig * tj;
                hn[e] = tanhf(c[e]) * og;
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
__global__ __launch_bounds__(NTHR) void decode_vae_kernel(const DecVaeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int per = H / U + 1;
    const int rb = blockIdx.x / per, role = blockIdx.x - rb * per;
    if (role == H / U) {
        head_body<H, MTW, kFlagStride>(a, rb, smem);
    } else {
        layer_body<H, MTW>(a, rb, role, smem);
    }
}

inline size_t layer_lds(int H, int mtw) {
    return (size_t)64 * H * 2 + (size_t)(8 / mtw) * mtw * 4 * 64 * 16 + (size_t)mtw * 256 * 2;
}
constexpr size_t kMaxLds = 160 * 1024;

template <int H, int MTW>
int launch(const DecVaeArgs& a, hipStream_t s) {
    const size_t lds = std::max(layer_lds(H, MTW), head_lds(H, a.noutp, MTW));
    if (lds > kMaxLds) return -2;
    const int grid = a.nrb * (H / U + 1);
    auto kern = decode_vae_kernel<H, MTW>;
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds) !=
            hipSuccess)
            return -9;
        attr = true;
    }
    if (!grid_fits((const void*)kern, NTHR, lds, grid)) return -8;
    const int nflags = a.nrb * kFlagStride;
    hipLaunchKernelGGL(zero_flags, dim3((nflags + 255) / 256), dim3(256), 0, s, a.flags, nflags);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NTHR), lds, s, a);
    return SKR_CHECK_LAUNCH();
}

}  // namespace

// Steps [t0, t1) of B sketches. Rows per row block: 16 * mtw (mtw 1 or 2).
// Eligible: H 256 with 1..32 mixtures, H 512 with 1..20 (the head's LDS).
// Returns 0 on success, < 0 on a rejected call (-2 geometry, -4 nrb, -6
// missing buffers, -8 grid not co-resident, -11 offsets past 32 bits).
SKR_API int skr_decode_vae(const DecVaeArgs* a, hipStream_t s) {
    if (a->N <= 0 || a->B <= 0 || a->t0 == a->t1) return 0;
    if (a->t0 < 0 || a->t1 > a->N || a->t0 > a->t1) return -2;
    if ((a->H != 256 && a->H != 512) || (a->mtw != 1 && a->mtw != 2)) return -2;
    if (a->M < 1 || a->M > (a->H == 256 ? 32 : 20) || a->nout != 3 + 6 * a->M ||
        a->noutp != (a->nout + 15) / 16 * 16)
        return -2;
    if (a->nrb != (a->B + 16 * a->mtw - 1) / (16 * a->mtw)) return -4;
    if (a->WT == nullptr || a->Wx == nullptr || a->zb == nullptr || a->c0 == nullptr || a->cT == nullptr ||
        a->hbuf == nullptr || a->WoT == nullptr || a->bo == nullptr || a->xin == nullptr || a->out == nullptr ||
        a->done == nullptr || a->seed == nullptr || a->flags == nullptr || a->err == nullptr)
        return -6;
    if ((int64_t)(a->N + 1) * a->B * a->H * 2 > 0x7fffffffLL || (int64_t)(a->N + 1) * a->B * kXLd * 4 > 0x7fffffffLL)
        return -11;
    if (a->H == 256) return a->mtw == 1 ? launch<256, 1>(*a, s) : launch<256, 2>(*a, s);
    return a->mtw == 1 ? launch<512, 1>(*a, s) : launch<512, 2>(*a, s);
}

SKR_API int skr_decode_vae_args_size() { return (int)sizeof(DecVaeArgs); }
