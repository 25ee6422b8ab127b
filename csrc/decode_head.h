// The parts the fused whole-sketch VAE decoders share (csrc/decode_vae.hip:
// plain lstm; csrc/decode_vae_ln.hip: layer_norm): the swizzled LDS staging
// of a bf16 weight matrix and the MDN head + sampler role of a row block.
//
// The head is a template over the launch's argument struct (both decoders'
// structs name the fields it reads alike) and over FS, the number of flag
// words per row block. In every layout words [0, H/16) are the layer
// workgroups' h epochs and word H/16 is the head's.
#pragma once
#include "handoff.h"
#include "mdn_sample.h"

namespace skr {

constexpr int U = 16;            // hidden units per layer workgroup
constexpr int NTHR = 512;        // 8 waves
constexpr int kXLd = 8;          // floats per fed-input row

// nrows x K of a row-major bf16 matrix into LDS, 16-byte chunks of LDS row r
// XOR-swizzled by (r & 15). GATE: LDS row r = gate (r >> 4), unit u0 + (r & 15)
// of a [4H][K] matrix; otherwise LDS row r = source row r.
template <bool GATE>
__device__ void stage(__hip_bfloat16* lds, const __hip_bfloat16* src, int nrows, int K, int H, int u0) {
    const int cpr = K / 8;
    for (int i = threadIdx.x; i < nrows * cpr; i += NTHR) {
        const int r = i / cpr, c = i - r * cpr;
        const int sr = GATE ? (r >> 4) * H + u0 + (r & 15) : r;
        const bf16x8 v = *(const bf16x8*)(src + (int64_t)sr * K + c * 8);
        *(bf16x8*)(lds + r * K + ((c ^ (r & 15)) * 8)) = v;
    }
}

__device__ __forceinline__ bf16x8 frag(const __hip_bfloat16* lds, int row, int K, int chunk) {
    return *(const bf16x8*)(lds + row * K + ((chunk ^ (row & 15)) * 8));
}

// ---------------------------------------------------------------------------------
// MDN head + sampler of a row block
// ---------------------------------------------------------------------------------
template <int H, int MTW, int FS, class Args>
__device__ void head_body(const Args& a, int rb, unsigned char* smem) {
    constexpr int RB = 16 * MTW, NKS = H / 32, NW = H / U, CW = 8 / MTW;
    const int noutp = a.noutp, NT = noutp / 16, ldz = noutp + 4;
    __hip_bfloat16* Wo = (__hip_bfloat16*)smem;                  // [noutp][H]
    float* zs = (float*)(smem + (int64_t)noutp * H * 2);         // [RB][ldz]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int B = a.B, N = a.N, M = a.M, nout = a.nout;
    constexpr int stop_col = 4;

    stage<false>(Wo, a.WoT, noutp, H, H, 0);
    __syncthreads();

    uint32_t* fl = a.flags + (int64_t)rb * FS;
    const uint32_t* top_flags = fl;
    uint32_t* my_flag = fl + NW;
    const __amdgpu_buffer_rsrc_t r_h = rsrc(a.hbuf, (int64_t)(N + 1) * B * H * 2);
    const __amdgpu_buffer_rsrc_t r_x = rsrc(a.xin, (int64_t)(N + 1) * B * kXLd * 4);
    // wave w: row tile w % MTW, column tiles w / MTW, + CW, + 2 CW, ...
    const int mt = w % MTW, j0 = w / MTW;
    const int row_t0 = rb * RB + mt * 16;
    const bool tile_on = row_t0 < B;
    const int arow = min(row_t0 + fr, B - 1);
    const int64_t seed = *a.seed;
    constexpr int RPW = RB / 8;         // sampled rows per wave: w, w + 8, ...
    bool fin[RPW];                      // row finished: emits padding from the next step
    int nf[RPW];
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int b = rb * RB + w + 8 * k;
        fin[k] = b < B && a.done[b] != 0;
        nf[k] = (b < B && a.nforced != nullptr) ? a.nforced[b] : 0;
    }
    // Row temperatures, once per launch, in ONE register: lane k holds that of the wave's k-th sampled
    // row, temps[b] (local row) or the launch's scalar; the draw reads it back with readlane. The scalar
    // goes in as a value first: written as a select between the two loads, the compiler selects between
    // their addresses, gives the kernel argument a scratch slot and the launch scratch memory.
    float tp = a.temp;
    asm volatile("" : "+v"(tp));
    {
        const int b = rb * RB + w + 8 * lane;
        if (lane < RPW && b < B && a.temps != nullptr) tp = a.temps[b];
    }
    const float itp = 1.f / tp;         // the reciprocal too: one division per launch, none per stroke
    bool ok = true;

    for (int t = a.t0; t < a.t1; ++t) {
        if (tile_on) {
            ok = ok && wait_flags(top_flags, NW, (uint32_t)(t + 1), a.err);
            bf16x8 af[NKS];
            const uint32_t base = (uint32_t)(((int64_t)(t + 1) * B + arow) * H * 2);
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) af[ks] = ld_sc1(r_h, base + (uint32_t)((ks * 32 + fq * 8) * 2));
            for (int j = j0; j < NT; j += CW) {
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks)
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], frag(Wo, j * 16 + fr, H, ks * 4 + fq), acc,
                                                                  0, 0, 0);
                const int col = j * 16 + fr;
                const float bv = col < nout ? a.bo[col] : 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) zs[(mt * 16 + 4 * fq + e) * ldz + col] = acc[e] + bv;
            }
        }
        __syncthreads();
        const uint32_t key = hash_key(seed, 0x5A3Du, (uint32_t)t);
        float row[RPW][5];
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
            const int r = w + 8 * k, b = rb * RB + r;
            if (b >= B) continue;   // wave-uniform
            const float* zr = zs + r * ldz;
            const float tk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tp), k));
            const float itk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(itp), k));
            const MdnDraw dr = mdn_sample_wave(zr, M, 1, tk, itk, a.greedy, 0, key, (uint32_t)(a.row0 + b), (uint32_t)t);
            const uint32_t xoff = (uint32_t)((((int64_t)(t + 1) * B + b) * kXLd) * 4);
            if (t < nf[k]) {          // prefix: the host's x(t+1) stands (wave-uniform)
#pragma unroll
                for (int c = 0; c < 5; ++c) row[k][c] = ld_sc1_f32(r_x, xoff + c * 4);
            } else {
#pragma unroll
                for (int c = 0; c < 5; ++c) row[k][c] = dr.row[c];
                if (lane < 5) {
                    const float v = lane == 0 ? dr.row[0] : lane == 1 ? dr.row[1] : lane == 2 ? dr.row[2]
                                  : lane == 3 ? dr.row[3] : dr.row[4];
                    st_sc1_f32(r_x, xoff + lane * 4, v);
                }
            }
            if (a.zout != nullptr)
                for (int c = lane; c < nout; c += 64) a.zout[((int64_t)t * B + b) * nout + c] = zr[c];
        }
        publish(my_flag, (uint32_t)(t + 1));
        // outputs no workgroup of this launch reads: stored after the hand-off
#pragma unroll
        for (int k = 0; k < RPW; ++k) {
            const int b = rb * RB + w + 8 * k;
            if (b >= B) continue;
            if (lane == 0) {
                float* o = a.out + ((int64_t)b * N + t) * 5;
#pragma unroll
                for (int c = 0; c < 5; ++c) o[c] = fin[k] ? (c == stop_col ? 1.f : 0.f) : row[k][c];
            }
            fin[k] = fin[k] || row[k][stop_col] > 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < RPW; ++k) {
        const int b = rb * RB + w + 8 * k;
        if (b < B && lane == 0) a.done[b] = fin[k] ? 1 : 0;
    }
    (void)ok;
}

inline size_t head_lds(int H, int noutp, int mtw) {
    return (size_t)noutp * H * 2 + (size_t)16 * mtw * (noutp + 4) * 4;
}

}  // namespace skr
