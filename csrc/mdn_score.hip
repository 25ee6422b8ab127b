// Per-sketch likelihood scores of the mixture-density head: the output
// projection on MFMA and the MDN terms summed PER SKETCH over its real
// positions, in one kernel. z = X @ W + b never reaches HBM and padded
// positions are never computed.
//
// X [T * B, Hd] is the time-major decoder output (fp32 or bf16 rows),
// tgt [T * B, 5] the targets, lengths [B] the number of real points. With
//   shape[t, b] = -logaddexp(log S, log eps),  pen[t, b] = CE(pen logits, target)
// (the per-row terms of csrc/mdn.hip / csrc/mdn_head.hip in Magenta mode,
// before their mask), the kernel returns
//   score[b][0] = sum_{t < len[b]} shape[t, b]
//   score[b][1] = sum_{t < len[b]} pen[t, b]  (+ pen[len[b], b] when include_end
//                                              and len[b] < T: the end-of-sketch row)
// The mask is a select on t against lengths: rows past a sketch's counted
// positions contribute exactly zero whatever they hold (NaN included).
//
// Geometry (mdn_head_score): a 4-wave workgroup owns the 16 sketches
// b0 .. b0 + 15 and the time slab [s * tps, (s + 1) * tps). A round covers 4
// time steps, one per wave: rows (t, b0 .. b0 + 15) are 16 consecutive rows of
// X, one v_mfma_f32_16x16x32_bf16 A tile. The W^T K chunks go through a
// double-buffered padded LDS tile shared by the four waves (as mdn_head_fwd).
// The z tile goes to LDS (reusing the staging buffers), one row per 32-lane
// half-wave, lane k = mixture component k; every half-wave keeps the two
// running sums of its 8 sketches in registers across the rounds.
//   * deterministic: fixed order over t in a wave, waves summed in wave
//     order, slabs in slab order (mdn_score_finish); no atomics
//   * a round at or past the largest counted position of the block's 16
//     sketches is never started, and a wave whose t is past it loads no X
//   * lanes of sketches b >= B read the clamped row B - 1 of their time step
//     (never the next step's rows) and count nothing
#include "common.h"

namespace {

using namespace skr;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxNoutP = 160;        // NOUTP = NOUT rounded up to 32 (M <= 24)
constexpr int kSk = 16;               // sketches per workgroup (one MFMA tile of rows)
constexpr int kWaves = 4;             // time steps per round
constexpr int kKC = 64;               // K chunk staged per LDS buffer
constexpr int kLdk = kKC + 8;         // padded LDS row (144 B): conflict-free fragment reads
constexpr int kWPieces = kMaxNoutP * (kKC / 8) / 256;   // 16-byte W^T pieces per thread per chunk (5)
constexpr float kLog2Pi = 1.8378770664093453f;

__device__ __forceinline__ float hw_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
    return v;
}
__device__ __forceinline__ float hw_max(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 32));
    return v;
}
__device__ __forceinline__ uint32_t pack_bf16(float a, float b) {
    return (uint32_t)__builtin_bit_cast(unsigned short, to_bf16(a)) |
           ((uint32_t)__builtin_bit_cast(unsigned short, to_bf16(b)) << 16);
}

struct HeadScore {
    const float* X; int64_t ldx;     // [T * B] rows (fp32, or bf16 when x_bf16), row stride ldx
    int Hd, x_bf16;
    const __hip_bfloat16* Wt;        // [NOUTP][Hd] bf16 (rows >= NOUT zero)
    const float* bias;               // [NOUT]
    const float* tgt; int64_t ldt;   // [T * B][5]
    const int64_t* lengths;          // [B]
    int T, B, M, NOUT, NOUTP, include_end;
    int tps, S;                      // time steps per slab (multiple of 4), slabs (S * tps >= T)
    float log_floor;                 // log eps
    float* part;                     // [S][B][2] per-slab sums
    float* score;                    // [B][2]
};

// X fragments of one K chunk for lane (fr, fq): row arow, k = kc * kKC +
// ks * 32 + fq * 8 .. +7 for ks = 0, 1 -- raw, converted at use
template <bool XB> struct XChunk { f32x4 v[2][2]; };
template <> struct XChunk<true> { u32x4 v[2]; };

template <bool XB>
__global__ __launch_bounds__(256) void mdn_head_score(const HeadScore a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __hip_bfloat16* Bs = (__hip_bfloat16*)smem;                 // [2][NOUTP][kLdk]
    float* zt = (float*)smem;                                     // [4 waves][16][NOUTP] (after the K loop)
    float* red = (float*)(smem + 2 * kMaxNoutP * kLdk * 2);       // [4 waves][16 sketches][2]
    int* lens = (int*)(red + kWaves * kSk * 2);                   // [16 sketches] (-1: no such sketch)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int hl = lane & 31, hh = lane >> 5;                     // half-wave lane / half-wave of the wave
    const int NOUTP = a.NOUTP, NC = NOUTP / 16, Hd = a.Hd, M = a.M, T = a.T, B = a.B;
    const int b0 = blockIdx.x * kSk;
    const int inc = a.include_end ? 1 : 0;
    // counted positions: shape at t < len, pen at t < len + inc (and t < T)
    int tmax = 0;
    for (int j = 0; j < kSk; ++j) {
        if (b0 + j < B) {
            const int len = (int)max((int64_t)0, min((int64_t)T, a.lengths[b0 + j]));
            tmax = max(tmax, min(T, len + inc));
        }
    }
    if (tid < kSk) lens[tid] = b0 + tid < B ? (int)max((int64_t)0, min((int64_t)T, a.lengths[b0 + tid])) : -1;
    const int t_begin = blockIdx.y * a.tps;
    const int t_end = min(min(T, t_begin + a.tps), tmax);         // past it: padding for all 16 sketches
    const int bcl = min(b0 + fr, B - 1);                           // clamped sketch of this lane's A row

    // running sums of sketch b0 + hh + 2 hl, held by lane hl < 8 of each half-wave
    float ss = 0.f, sp = 0.f;

    const int nchunks = Hd / kKC, npieces = NOUTP * (kKC / 8);
    u32x4 wr[kWPieces];
    XChunk<XB> xr;
    auto load_w = [&](int kc) {
#pragma unroll
        for (int j = 0; j < kWPieces; ++j) {
            const int p = tid + 256 * j;
            if (p < npieces) wr[j] = *(const u32x4*)(a.Wt + (int64_t)(p >> 3) * Hd + kc * kKC + (p & 7) * 8);
        }
    };
    auto store_w = [&](int buf) {
        __hip_bfloat16* dst = Bs + buf * kMaxNoutP * kLdk;
#pragma unroll
        for (int j = 0; j < kWPieces; ++j) {
            const int p = tid + 256 * j;
            if (p < npieces) *(u32x4*)(dst + (p >> 3) * kLdk + (p & 7) * 8) = wr[j];
        }
    };
    auto load_x = [&](int64_t arow, int kc) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int64_t o = arow * a.ldx + kc * kKC + ks * 32 + fq * 8;
            if constexpr (XB) {
                xr.v[ks] = *(const u32x4*)((const __hip_bfloat16*)(const void*)a.X + o);
            } else {
                xr.v[ks][0] = *(const f32x4*)(a.X + o);
                xr.v[ks][1] = *(const f32x4*)(a.X + o + 4);
            }
        }
    };
    auto frag = [&](int ks) -> bf16x8 {
        if constexpr (XB) {
            return __builtin_bit_cast(bf16x8, xr.v[ks]);
        } else {
            const f32x4 lo = xr.v[ks][0], hi = xr.v[ks][1];
            const u32x4 pk = {pack_bf16(lo[0], lo[1]), pack_bf16(lo[2], lo[3]), pack_bf16(hi[0], hi[1]),
                              pack_bf16(hi[2], hi[3])};
            return __builtin_bit_cast(bf16x8, pk);
        }
    };

    for (int t0 = t_begin; t0 < t_end; t0 += kWaves) {
        const int t = t0 + w;
        const bool live = t < t_end;                              // wave-uniform: no load of X past the counted rows
        const int64_t arow = (int64_t)(live ? t : t0) * B + bcl;
        f32x4 acc[kMaxNoutP / 16];
#pragma unroll
        for (int c = 0; c < kMaxNoutP / 16; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        // K loop: W^T chunk kc in LDS buffer kc & 1, chunk kc + 1 in registers
        // (stored while chunk kc is consumed), X chunk kc + 1 loaded before
        // the MFMAs of chunk kc
        load_w(0);
        store_w(0);
        if (1 < nchunks) load_w(1);
        if (live) load_x(arow, 0);
        __syncthreads();
        for (int kc = 0; kc < nchunks; ++kc) {
            if (kc + 1 < nchunks) {
                store_w((kc + 1) & 1);
                if (kc + 2 < nchunks) load_w(kc + 2);
            }
            if (live) {
                const bf16x8 A0 = frag(0), A1 = frag(1);
                if (kc + 1 < nchunks) load_x(arow, kc + 1);
                const __hip_bfloat16* Bc = Bs + (kc & 1) * kMaxNoutP * kLdk;
#pragma unroll
                for (int ks = 0; ks < kKC / 32; ++ks) {
                    const bf16x8 A = ks == 0 ? A0 : A1;
#pragma unroll
                    for (int c = 0; c < kMaxNoutP / 16; ++c) {
                        if (c < NC) {
                            const bf16x8 Bf = *(const bf16x8*)(Bc + (c * 16 + fr) * kLdk + ks * 32 + fq * 8);
                            acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, Bf, acc[c], 0, 0, 0);
                        }
                    }
                }
            }
            __syncthreads();
        }
        // ---- this wave's z tile (+bias) into LDS (reuses the staging buffers)
        float* zw = zt + w * kSk * NOUTP;
        if (live) {
#pragma unroll
            for (int c = 0; c < kMaxNoutP / 16; ++c) {
                if (c < NC) {
                    const int col = c * 16 + fr;
                    const float bv = col < a.NOUT ? a.bias[col] : 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) zw[(4 * fq + e) * NOUTP + col] = acc[c][e] + bv;
                }
            }
        }
        __syncthreads();
        // ---- per-row MDN terms: one row per half-wave, lane k = component k
        //      (the math of mdn_head_fwd / csrc/mdn.hip, Magenta mode)
        if (live) {
#pragma unroll 1
            for (int i = 0; i < kSk / 2; ++i) {
                const int rr = hh + 2 * i;
                const int len = lens[rr];
                if (t >= len + inc) continue;                      // not counted: nothing read (half-wave uniform)
                const float* zr = zw + rr * NOUTP;
                const float* tr = a.tgt + ((int64_t)t * B + b0 + rr) * a.ldt;
                const bool on = hl < M;
                const float x1 = tr[0], x2 = tr[1];
                const float p0 = tr[2], p1 = tr[3], p2 = tr[4];
                const float zpi = on ? zr[3 + hl] : -INFINITY;
                const float mpi = hw_max(zpi);
                const float epi = on ? __expf(zpi - mpi) : 0.f;
                const float spi = hw_sum(epi);
                const float logpi = zpi - mpi - __logf(spi);
                float lp = -INFINITY;
                if (on) {
                    const float mu1 = zr[3 + M + hl], mu2 = zr[3 + 2 * M + hl];
                    const float ls1 = zr[3 + 3 * M + hl], ls2 = zr[3 + 4 * M + hl];
                    const float rho = tanhf(zr[3 + 5 * M + hl]);
                    const float s1 = expf(ls1);
                    const float s2 = expf(ls2);
                    const float n1 = (x1 - mu1) / s1;
                    const float n2 = (x2 - mu2) / s2;
                    const float om = 1.f - rho * rho;
                    const float Z = n1 * n1 + n2 * n2 - 2.f * rho * n1 * n2;
                    lp = logpi - Z / (2.f * om) - kLog2Pi - ls1 - ls2 - 0.5f * logf(om);
                }
                const float mlp = hw_max(lp);
                const float elp = on ? expf(lp - mlp) : 0.f;
                const float slp = hw_sum(elp);
                const float logS = mlp + logf(slp);
                const float mx = fmaxf(logS, a.log_floor), mn = fminf(logS, a.log_floor);
                const float lae = mx + log1pf(expf(mn - mx));
                const float l0 = zr[0], l1 = zr[1], l2 = zr[2];
                const float ml = fmaxf(l0, fmaxf(l1, l2));
                const float e0 = expf(l0 - ml), e1 = expf(l1 - ml), e2 = expf(l2 - ml);
                const float se = e0 + e1 + e2, lse = ml + logf(se);
                const float ce = -(p0 * (l0 - lse) + p1 * (l1 - lse) + p2 * (l2 - lse));
                if (hl == i) {
                    ss += t < len ? -lae : 0.f;                    // the end-of-sketch row has no shape term
                    sp += ce;
                }
            }
        }
        __syncthreads();   // every wave is done with the z tile before the next round stages W^T
    }
    // ---- the four waves' sums, in wave order
    if (hl < kSk / 2) {
        red[(w * kSk + hh + 2 * hl) * 2] = ss;
        red[(w * kSk + hh + 2 * hl) * 2 + 1] = sp;
    }
    __syncthreads();
    if (tid < 2 * kSk) {
        const int j = tid >> 1, k = tid & 1;
        float v = red[j * 2 + k];
#pragma unroll
        for (int q = 1; q < kWaves; ++q) v += red[(q * kSk + j) * 2 + k];
        if (b0 + j < B) a.part[((int64_t)blockIdx.y * B + b0 + j) * 2 + k] = v;
    }
}

// score[b][k] = sum over the S slabs, in slab order
__global__ __launch_bounds__(256) void mdn_score_finish(const float* part, int S, int n, float* score) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (int s = 0; s < S; ++s) v += part[(int64_t)s * n + i];
    score[i] = v;
}

inline size_t score_lds() { return (size_t)2 * kMaxNoutP * kLdk * 2 + (size_t)kWaves * kSk * 2 * 4 + kSk * 4; }

}  // namespace

SKR_API int skr_mdn_head_score(const HeadScore* a, hipStream_t s) {
    if (a->M < 1 || a->M > 24 || a->NOUT != 3 + 6 * a->M || a->NOUTP % 32 || a->NOUTP < a->NOUT ||
        a->NOUTP > kMaxNoutP)
        return -2;
    if (a->Hd <= 0 || a->Hd % kKC != 0 || a->ldx < a->Hd || a->ldx % (a->x_bf16 ? 8 : 4) != 0 ||
        ((uintptr_t)a->X & 15) || ((uintptr_t)a->Wt & 15) || a->ldt < 5)
        return -3;
    if (a->T < 1 || a->B < 1 || a->tps < kWaves || a->tps % kWaves || a->S < 1 ||
        (int64_t)a->S * a->tps < a->T || a->S > 65535)
        return -4;
    static bool attr = false;
    if (!attr) {
        if (hipFuncSetAttribute((const void*)mdn_head_score<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)score_lds()) != hipSuccess ||
            hipFuncSetAttribute((const void*)mdn_head_score<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)score_lds()) != hipSuccess)
            return -9;
        attr = true;
    }
    // the four z tiles reuse the staging buffers
    static_assert((size_t)kWaves * kSk * kMaxNoutP * 4 <= (size_t)2 * kMaxNoutP * kLdk * 2, "z tiles fit");
    const dim3 grid((a->B + kSk - 1) / kSk, a->S);
    if (a->x_bf16) hipLaunchKernelGGL(mdn_head_score<true>, grid, dim3(256), score_lds(), s, *a);
    else hipLaunchKernelGGL(mdn_head_score<false>, grid, dim3(256), score_lds(), s, *a);
    const int n = 2 * a->B;
    hipLaunchKernelGGL(mdn_score_finish, dim3((n + 255) / 256), dim3(256), 0, s, a->part, a->S, n, a->score);
    return SKR_CHECK_LAUNCH();
}

SKR_API int skr_mdn_head_score_args_size() { return (int)sizeof(HeadScore); }
