// Training batches assembled on the device: a stateless epoch shuffle picks
// the sketches, each is scaled per axis, interior points of its strokes are
// dropped and merged into the kept point before them, and the rows are padded
// to magenta stroke-5 with the start token.
//
// The definition lives in sketch_rnn_amd/ops/batch.py; every random draw is a
// hash of (seed, stream, step, index) from common.h, so a batch is a pure
// function of its arguments.
//
// One launch, one wave per batch row, no global atomics, no waits across
// workgroups, no scratch.
//
//   select   every lane runs the same cycle-walking Feistel permutation of the
//            row's position in its epoch (wave-uniform inputs, no divergence).
//   stage    64 points per pass: the scaled offsets go to LDS; the ballot of
//            the lift flags gives each point the first index of its stroke
//            (carried across passes), hence its eligibility; the ballot of
//            the kept points gives each its output row (running total), whose
//            source index goes to LDS beside the drop masks.
//   output   the row's 5 (Nmax + 1) dwords, one per lane per pass, so every
//            store instruction covers 256 contiguous bytes whatever the row
//            stride. The lanes of the x and y columns walk the dropped
//            followers of their kept point in LDS and add them in fp64 in
//            ascending order, as the host loop does.
//
// LDS per row: 10 B per point and two 8-byte masks per 64 points, 20.5 KiB at
// Nmax = 2048.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxN = 2048;

struct BatchArgs {
    const float* points;      // [P, 3] (dx, dy, lift)
    const int64_t* offsets;   // [S + 1]
    const int64_t* labels_in; // [S]
    const int64_t* indices;   // [B] or null: the shuffle
    float* strokes;           // [B, Nmax + 1, 5]
    int64_t* lengths;         // [B]
    int64_t* labels;          // [B]
    int64_t S, seed, step, row0, G;
    double prob;
    float f;
    int B, Nmax, kbits;
    uint32_t s_shuffle, s_scale, s_drop;   // stream ids
};

// Position p of an epoch -> sketch index: four Feistel rounds on 2 kbits bits,
// walked until the value falls below S.
__device__ __forceinline__ uint32_t shuffle_index(uint32_t p, uint32_t S, uint32_t key, int k) {
    const uint32_t mask = (1u << k) - 1u;
    uint32_t x = p;
    do {
        uint32_t L = x >> k, R = x & mask;
#pragma unroll
        for (uint32_t r = 0; r < 4u; ++r) {
            const uint32_t nr = L ^ (skr::mix32(R ^ skr::mix32(key + r)) & mask);
            L = R;
            R = nr;
        }
        x = (L << k) | R;
    } while (x >= S);
    return x;
}

__global__ __launch_bounds__(64) void batch_kernel(BatchArgs a) {
    extern __shared__ unsigned long long s_mem[];
    const int Nmax = a.Nmax, chunks = (Nmax + 63) >> 6;
    unsigned long long* s_dropm = s_mem;                 // dropped points of rows 64 c .. 64 c + 63
    unsigned long long* s_liftm = s_mem + chunks;        // lifted points
    float* s_x = reinterpret_cast<float*>(s_mem + 2 * chunks);
    float* s_y = s_x + Nmax;
    unsigned short* s_idx = reinterpret_cast<unsigned short*>(s_y + Nmax);   // output row -> source row
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t g = a.row0 + b;

    // selection (wave-uniform)
    int64_t idx;
    if (a.indices) {
        idx = a.indices[b];
    } else {
        const int64_t q = a.step * a.G + g;
        const int64_t epoch = q / a.S;
        const uint32_t p = (uint32_t)(q - epoch * a.S);
        idx = shuffle_index(p, (uint32_t)a.S, skr::hash_key(a.seed, a.s_shuffle, (uint32_t)epoch), a.kbits);
    }
    const bool ok = idx >= 0 && idx < a.S;
    int64_t o0 = 0;
    int n = 0;
    if (ok) {
        o0 = a.offsets[idx];
        const int64_t len = a.offsets[idx + 1] - o0;
        n = (int)(len < 0 ? 0 : (len > Nmax ? Nmax : len));
    }

    // per-axis scale: single fp32 operations
    const uint32_t ks = skr::hash_key(a.seed, a.s_scale, (uint32_t)a.step);
    const uint32_t kd = skr::hash_key(a.seed, a.s_drop, (uint32_t)a.step);
    const float ux = skr::hash_uniform(ks, (uint32_t)(2 * g));
    const float uy = skr::hash_uniform(ks, (uint32_t)(2 * g + 1));
    const float sx = ((ux - 0.5f) * 2.0f) * a.f + 1.0f;
    const float sy = ((uy - 0.5f) * 2.0f) * a.f + 1.0f;
    const uint32_t dbase = (uint32_t)(g * (int64_t)Nmax);

    // stage
    const float* src = a.points + o0 * 3;
    const unsigned long long below = (1ull << lane) - 1ull;
    int first = 0;                      // first index of the stroke that enters this pass
    unsigned long long prev_lift = 1ull;   // lift of the row before this pass; row -1 counts as lifted
    int kept = 0;
    for (int c = 0; c < chunks; ++c) {
        const int t = c * 64 + lane;
        const bool in = t < n;
        float x = 0.f, y = 0.f;
        bool lift = false;
        if (in) {
            x = src[(int64_t)t * 3] * sx;
            y = src[(int64_t)t * 3 + 1] * sy;
            lift = src[(int64_t)t * 3 + 2] == 1.0f;
        }
        const unsigned long long lm = __ballot(lift);
        const unsigned long long starts = (lm << 1) | prev_lift;     // bit r: row r starts a stroke
        const unsigned long long upto = starts & (below | (1ull << lane));
        const int fst = upto ? c * 64 + 63 - __clzll((long long)upto) : first;
        const bool plift = (starts >> lane) & 1ull;
        bool drop = false;
        if (in && !lift && !plift && t - fst > 2) {
            const float u = skr::hash_uniform(kd, dbase + (uint32_t)t);
            drop = (double)u < a.prob;
        }
        const unsigned long long dm = __ballot(drop);
        const unsigned long long km = __ballot(in && !drop);
        if (t < Nmax) {
            s_x[t] = x;
            s_y[t] = y;
        }
        if (in && !drop) s_idx[kept + __popcll(km & below)] = (unsigned short)t;
        if (lane == 0) {
            s_dropm[c] = dm;
            s_liftm[c] = lm;
        }
        kept += __popcll(km);
        if (starts) first = c * 64 + 63 - __clzll((long long)starts);
        prev_lift = lm >> 63;
    }
    __syncthreads();

    // output
    const int W = 5 * (Nmax + 1);
    float* orow = a.strokes + (int64_t)b * W;
    for (int e = lane; e < W; e += 64) {
        const int j1 = (int)((unsigned)e / 5u), col = e - 5 * j1;
        float v;
        if (j1 == 0) {
            v = col == 2 ? 1.f : 0.f;
        } else if (j1 - 1 < kept) {
            const int k = s_idx[j1 - 1];
            if (col < 2) {
                const float* s = col == 0 ? s_x : s_y;
                double acc = (double)s[k];
                for (int t = k + 1; t < n && ((s_dropm[t >> 6] >> (t & 63)) & 1ull); ++t) acc += (double)s[t];
                v = (float)acc;
            } else {
                const bool lift = (s_liftm[k >> 6] >> (k & 63)) & 1ull;
                v = col == 4 ? 0.f : ((col == 3) == lift ? 1.f : 0.f);
            }
        } else {
            v = col == 4 ? 1.f : 0.f;
        }
        orow[e] = v;
    }
    if (lane == 0) {
        a.lengths[b] = kept;
        a.labels[b] = ok ? a.labels_in[idx] : 0;
    }
}

}  // namespace

SKR_API int skr_batch_assemble(const BatchArgs* a, hipStream_t s) {
    if (a->B < 0 || a->Nmax < 1 || a->Nmax > kMaxN) return -2;
    if (a->S < 1 || a->S > (1ll << 30) || a->kbits < 1 || a->kbits > 15 || (1ll << (2 * a->kbits)) < a->S) return -3;
    if (a->G < 1 || a->row0 < 0 || a->step < 0 || !(a->prob >= 0.0 && a->prob <= 1.0) || !(a->f >= 0.f && a->f < 1.f))
        return -3;
    if (a->B == 0) return 0;
    if (!a->points || !a->offsets || !a->labels_in || !a->strokes || !a->lengths || !a->labels) return -4;
    const int chunks = (a->Nmax + 63) / 64;
    const size_t lds = (size_t)chunks * 16 + (size_t)a->Nmax * 10 + 8;
    hipLaunchKernelGGL(batch_kernel, dim3(a->B), dim3(64), lds, s, *a);
    return SKR_CHECK_LAUNCH();
}

SKR_API int skr_batch_args_size() { return (int)sizeof(BatchArgs); }
