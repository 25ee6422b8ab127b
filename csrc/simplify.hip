// Ramer-Douglas-Peucker tolerances of a batch of stroke sequences, and the
// simplified batch at a per-sketch epsilon or fitted to a length.
//
// The definition lives in sketch_rnn_amd/ops/simplify.py: points are the
// running sum of the offsets, a run ends at a lifted row or at the last row,
// tol[t] is the largest epsilon at which RDP still keeps point t (+inf at the
// ends of a run, -inf at and past the length), RDP at epsilon keeps
// {t : tol[t] > epsilon} and the run ends, and the fit is the smallest
// tolerance value that leaves at most max_len points.
//
// One launch, one workgroup per sketch, two points per thread, no global
// atomics, no waits across workgroups, no scratch; rows at or past the length
// are never read.
//
//   points     every wave scans its 64 offsets in fp64; the waves' totals go
//              through LDS. The ballot of the run ends of every 64 rows gives
//              each point its run (s, e).
//   recursion  level by level. Every unresolved point holds its segment
//              (l, r) and its cap in registers, computes its key and does an
//              LDS atomicMax of the key's bit pattern (non-negative doubles
//              order as unsigned integers) into the slot of l; after a barrier
//              the points whose key is the maximum do an atomicMin of their
//              index; after a second barrier the winner takes
//              tol = min(cap, d) and the others move to (l, m) or (m, r) with
//              that cap. Every point of the segment computes d from the slot's
//              key itself, with the winner's operations. Integer max and min
//              do not depend on the order, so the result is the same bits in
//              every run. The slots alternate between two sets by the parity
//              of the level: a slot read at one level is cleared during the
//              next, when its set is idle, which saves a barrier per level.
//   fit        a bisection over the bit pattern of tol between epsilon and
//              +inf, one block-wide count per step, only for a sketch that
//              epsilon alone leaves too long.
//   output     the kept indices are compacted in sequence order (ballots and
//              the waves' counts through LDS); row i then takes
//              fp32(P_{k_i} - P_{k_{i-1}}), the difference in fp64, and the
//              pen columns of row k_i; the rows past the new length are padded.
//
// LDS per point: 16 B of coordinates and two slot sets of 12 B: 40 B, so
// 20 KiB for the 512-point tier (8 workgroups of 4 waves per CU) and 80 KiB
// for the 2048-point tier (2 workgroups of 16 waves, the CU's 32 waves).
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxN = 2048;
constexpr int kPer = 2;                 // points per thread
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;

struct RdpArgs {
    const float* strokes;     // [B, N, D]
    const int64_t* lengths;   // [B]
    const double* epsilon;    // [B]; needed with out
    double* tol;              // [B, N] or null
    float* out;               // [B, N, D] or null: tolerances only
    int64_t* new_lengths;     // [B], with out
    double* eps_used;         // [B], with out
    int* rounds;              // [B] or null: levels of the recursion
    int B, N, D;
    int max_len;              // 0: no fit
};

__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < skr::kWave; o <<= 1) {
        const double u = __shfl_up(v, o, skr::kWave);
        if (lane >= o) v += u;
    }
    return v;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS, 8) void rdp_kernel(RdpArgs a) {
    constexpr int NMAX = THREADS * kPer, WAVES = THREADS / skr::kWave, CHUNKS = NMAX / skr::kWave;
    __shared__ double s_px[NMAX], s_py[NMAX];
    __shared__ unsigned long long s_bk[2][NMAX];   // largest key of the segment that starts here
    __shared__ int s_bi[2][NMAX];                  // lowest index with that key
    // The small tables live in the second index set while it is idle (before
    // and after the recursion), so that the 2048-point tier stays at 80 KiB.
    unsigned long long* s_ends = reinterpret_cast<unsigned long long*>(s_bi[1]);   // run ends of rows 64 c .. 64 c + 63
    double* s_wx = reinterpret_cast<double*>(s_bi[1]) + CHUNKS;
    double* s_wy = s_wx + WAVES;
    int (*s_cnt)[CHUNKS] = reinterpret_cast<int (*)[CHUNKS]>(s_bi[1]);
    static_assert((CHUNKS + 2 * WAVES) * 8 <= NMAX * 4 && 2 * CHUNKS <= NMAX, "the small tables fit the idle set");
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int D = a.D, lift_col = a.D == 5 ? 3 : 2;
    const int64_t len = a.lengths[b];
    const int L = (int)(len < 0 ? 0 : (len > a.N ? a.N : len));
    const float* row = a.strokes + (int64_t)b * a.N * D;

    // points and run ends
    double cx = 0.0, cy = 0.0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int t = k * THREADS + tid;
        double dx = 0.0, dy = 0.0;
        bool end = false;
        if (t < L) {
            dx = (double)row[(int64_t)t * D];
            dy = (double)row[(int64_t)t * D + 1];
            end = row[(int64_t)t * D + lift_col] >= 0.5f || t == L - 1;
        }
        const double ix = wave_incl_scan(dx, lane), iy = wave_incl_scan(dy, lane);
        const unsigned long long m = __ballot(end);
        if (lane == 63) s_wx[w] = ix, s_wy[w] = iy;
        if (lane == 0) s_ends[k * WAVES + w] = m;
        __syncthreads();
        double ox = cx, oy = cy;
#pragma unroll 4
        for (int j = 0; j < WAVES; ++j) {
            const double wx = s_wx[j], wy = s_wy[j];
            if (j < w) ox += wx, oy += wy;
            cx += wx, cy += wy;
        }
        s_px[t] = ox + ix;
        s_py[t] = oy + iy;
        __syncthreads();
    }

    // every point's run (s, e); the ends of a run are resolved from the start
    int l[kPer], r[kPer], clr[kPer];
    double cap[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int t = k * THREADS + tid, c = k * WAVES + w;
        l[k] = r[k] = t;
        clr[k] = -1;
        cap[k] = t < L ? INFINITY : -INFINITY;
        if (t < L) {
            const unsigned long long m = s_ends[c];
            const unsigned long long below = m & ((1ull << lane) - 1ull), above = m >> lane;
            int s = 0, e = L - 1;
            if (below) {
                s = c * 64 + 64 - __clzll((long long)below);
            } else {
                for (int cc = c - 1; cc >= 0; --cc) {
                    const unsigned long long mm = s_ends[cc];
                    if (mm) {
                        s = cc * 64 + 64 - __clzll((long long)mm);
                        break;
                    }
                }
            }
            if (above) {
                e = t + __ffsll((unsigned long long)above) - 1;
            } else {
                for (int cc = c + 1; cc < CHUNKS; ++cc) {
                    const unsigned long long mm = s_ends[cc];
                    if (mm) {
                        e = cc * 64 + __ffsll((unsigned long long)mm) - 1;
                        break;
                    }
                }
            }
            if (t != s && t != e) l[k] = s, r[k] = e;
        }
    }

    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int t = k * THREADS + tid;
        s_bk[0][t] = s_bk[1][t] = 0ull;
        s_bi[0][t] = s_bi[1][t] = INT_MAX;
    }
    __syncthreads();

    // the recursion, one level per pass; a point is unresolved while l < r
    int rounds = 0;
    for (int par = 0;; par ^= 1) {
        double uu[kPer], key[kPer];
        int active = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (l[k] < r[k]) {
                const int t = k * THREADS + tid;
                const double lx = s_px[l[k]], ly = s_py[l[k]];
                const double ux = s_px[r[k]] - lx, uy = s_py[r[k]] - ly;
                const double vx = s_px[t] - lx, vy = s_py[t] - ly;
                uu[k] = ux * ux + uy * uy;
                key[k] = uu[k] > 0.0 ? fabs(ux * vy - uy * vx) : vx * vx + vy * vy;
                atomicMax(&s_bk[par][l[k]], (unsigned long long)__double_as_longlong(key[k]));
                active = 1;
            }
        }
        // The slot of the last index is never a segment's (a segment's left end
        // has two points after it): it carries "some point is unresolved".
        if (active) s_bi[par][NMAX - 1] = 0;
        __syncthreads();
        if (s_bi[par][NMAX - 1] != 0) break;
        ++rounds;
        if (tid == 0) s_bi[par ^ 1][NMAX - 1] = INT_MAX;
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (clr[k] >= 0) {          // the slot this point read at the level before
                s_bk[par ^ 1][clr[k]] = 0ull;
                s_bi[par ^ 1][clr[k]] = INT_MAX;
                clr[k] = -1;
            }
            if (l[k] < r[k] && (unsigned long long)__double_as_longlong(key[k]) == s_bk[par][l[k]])
                atomicMin(&s_bi[par][l[k]], k * THREADS + tid);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            if (l[k] < r[k]) {
                const int t = k * THREADS + tid;
                const int m = min(s_bi[par][l[k]], L - 1);
                const double kmax = __longlong_as_double((long long)s_bk[par][l[k]]);
                const double d = uu[k] > 0.0 ? __ddiv_rn(kmax, __dsqrt_rn(uu[k])) : __dsqrt_rn(kmax);
                cap[k] = fmin(cap[k], d);
                clr[k] = l[k];
                if (t == m) l[k] = r[k] = t;
                else if (t < m) r[k] = m;
                else l[k] = m;
            }
        }
    }
    if (a.rounds && tid == 0) a.rounds[b] = rounds;
    if (a.tol) {
#pragma unroll
        for (int k = 0; k < kPer; ++k) {
            const int t = k * THREADS + tid;
            if (t < a.N) a.tol[(int64_t)b * a.N + t] = cap[k];
        }
    }
    if (!a.out) return;

    // bit patterns of the tolerances; 0 past the length, which no threshold counts
    unsigned long long tb[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        tb[k] = k * THREADS + tid < L ? (unsigned long long)__double_as_longlong(cap[k]) : 0ull;
    double eps = a.epsilon[b];
    if (!(eps >= 0.0)) eps = 0.0;
    int cpar = 0;
    auto count_above = [&](unsigned long long e) {
        int c = 0;
#pragma unroll
        for (int k = 0; k < kPer; ++k) c += __popcll(__ballot(tb[k] > e));
        if (lane == 0) s_cnt[cpar][w] = c;
        __syncthreads();
        int tot = 0;
#pragma unroll 4
        for (int j = 0; j < WAVES; ++j) tot += s_cnt[cpar][j];
        cpar ^= 1;
        return tot;
    };
    if (a.max_len > 0) {
        unsigned long long lo = (unsigned long long)__double_as_longlong(eps), hi = kInfBits;
        if (lo < hi && count_above(lo) > a.max_len) {
            // count(lo) > max_len >= count(hi): the smallest threshold that fits is a tolerance value
            while (hi - lo > 1ull) {
                const unsigned long long mid = lo + (hi - lo) / 2ull;
                if (count_above(mid) > a.max_len) lo = mid;
                else hi = mid;
            }
            eps = __longlong_as_double((long long)hi);
        }
    }
    __syncthreads();

    // kept points in sequence order: the run ends stay at every epsilon
    const unsigned long long eb = (unsigned long long)__double_as_longlong(eps);
    int* s_idx = s_bi[0];
    bool keep[kPer];
    unsigned long long km[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        keep[k] = tb[k] > eb || tb[k] == kInfBits;
        km[k] = __ballot(keep[k]);
        if (lane == 0) s_cnt[0][k * WAVES + w] = __popcll(km[k]);
    }
    __syncthreads();
    int total = 0;
    int off[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) off[k] = 0;
#pragma unroll 4
    for (int j = 0; j < CHUNKS; ++j) {
        const int c = s_cnt[0][j];
#pragma unroll
        for (int k = 0; k < kPer; ++k) off[k] += j < k * WAVES + w ? c : 0;
        total += c;
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (keep[k]) s_idx[off[k] + __popcll(km[k] & ((1ull << lane) - 1ull))] = k * THREADS + tid;
    __syncthreads();
    float* orow = a.out + (int64_t)b * a.N * D;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        const int i = k * THREADS + tid;
        if (i >= a.N) continue;
        float* o = orow + (int64_t)i * D;
        if (i < total) {
            const int ki = s_idx[i];
            double qx = 0.0, qy = 0.0;
            if (i > 0) qx = s_px[s_idx[i - 1]], qy = s_py[s_idx[i - 1]];
            o[0] = (float)(s_px[ki] - qx);
            o[1] = (float)(s_py[ki] - qy);
            for (int c = 2; c < D; ++c) o[c] = row[(int64_t)ki * D + c];
        } else {
            for (int c = 0; c < D; ++c) o[c] = c == 4 ? 1.f : 0.f;
        }
    }
    if (tid == 0) {
        a.new_lengths[b] = total;
        a.eps_used[b] = eps;
    }
}

}  // namespace

SKR_API int skr_rdp(const RdpArgs* a, hipStream_t s) {
    if (a->B < 0 || a->N < 0 || (a->D != 3 && a->D != 5) || a->max_len < 0) return -2;
    if (a->N > kMaxN) return -3;
    if (a->B == 0) return 0;
    if (!a->lengths || (a->N > 0 && !a->strokes) || (!a->out && !a->tol) ||
        (a->out && (!a->epsilon || !a->new_lengths || !a->eps_used)))
        return -4;
    if (a->N <= 512) hipLaunchKernelGGL(rdp_kernel<256>, dim3(a->B), dim3(256), 0, s, *a);
    else hipLaunchKernelGGL(rdp_kernel<1024>, dim3(a->B), dim3(1024), 0, s, *a);
    return SKR_CHECK_LAUNCH();
}

SKR_API int skr_rdp_args_size() { return (int)sizeof(RdpArgs); }
