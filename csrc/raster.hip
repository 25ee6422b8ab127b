// Rasterise a batch of stroke sequences into [B, S, S] ink images.
//
// The definition lives in sketch_rnn_amd/ops/raster.py (rasterize_torch):
// points are the running sum of the offsets from the origin, segment
// P_t -> P_{t+1} is drawn iff 1 <= t < L and lift[t-1] < 0.5, the frame
// (scale, ox, oy) fits the points' bounding box into the canvas less a
// padding, and ink = clamp(width / 2 + 0.5 - d, 0, 1) with d the distance from
// the pixel centre (j + 0.5, i + 0.5) to the nearest drawn segment.
//
// Two launches, no atomics, no in-launch waits, no scratch:
//
//   raster_geom   one wave per sketch. Pass 1 scans the offsets for the
//                 bounding box and fits the frame; pass 2 scans them again and
//                 writes the drawn segments, compacted in sequence order, in
//                 pixel coordinates (fp32 [B, N, 4]) with their count. Rows
//                 at or past the length are never read. The scan, the box
//                 and the point transform are fp64 (a few hundred values per
//                 sketch), so the order of the scan does not show in the
//                 fp32 result; the frame is rounded to fp32 BEFORE it is
//                 applied, so a call that is handed the returned frame
//                 reproduces the fitted call bit for bit.
//   raster_tile   grid (tiles, B), one 256-thread workgroup per 16 x 16 pixel
//                 tile, one pixel per thread. The sketch's segments are read
//                 in chunks of kChunk; a segment whose bounding box lies
//                 further than the ink radius from the tile's pixel centres is
//                 dropped (it contributes exactly 0), the others are compacted
//                 into LDS in sequence order as (a, b - a, 1 / |b - a|^2), and
//                 every pixel takes the min squared distance over them. A
//                 pixel-segment distance is the same bits wherever the segment
//                 sits in that list (see the loop), so culling changes no bit.
//
// Tile shape: a square tile culls best for a given pixel count, and 256
// threads with 10 KiB of LDS keep 8 workgroups (32 waves, the CU's cap)
// resident within the 160 KiB of LDS. A wave covers 4 rows of 16 pixels, so
// its store is four 64-byte runs.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 16;               // pixels per tile edge
constexpr int kThreads = kTile * kTile; // one pixel per thread
constexpr int kWaves = kThreads / skr::kWave;
constexpr int kChunk = 512;             // segments tested per staging round trip
constexpr int kMaxS = 512;
constexpr int kMaxGridY = 65535;

struct RasterArgs {
    const float* strokes;     // [B, N, D]
    const int64_t* lengths;   // [B]
    const float* frame_in;    // [B, 3] or null: fit the frame
    float* frame;             // [B, 3] the frame used
    float* seg;               // [B, N, 4] drawn segments (ax, ay, bx, by) in pixels, compacted
    int* count;               // [B] drawn segments per sketch
    float* out;               // [B, S, S]
    int B, N, D, S;
    float width, pad;
    int cull;
    int b0;                   // first sketch of this tile launch
};

__device__ __forceinline__ double wave_incl_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < skr::kWave; o <<= 1) {
        const double u = __shfl_up(v, o, skr::kWave);
        if (lane >= o) v += u;
    }
    return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, skr::kWave));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, skr::kWave));
    return v;
}

// End point P_{t+1} and start point P_t of this lane's row t = base + lane,
// given the running point `carry` before the chunk; rows at or past L add 0.
struct ChunkPoints { double sx, sy, ex, ey; };

__device__ __forceinline__ ChunkPoints scan_chunk(const float* row, int D, int base, int L, int lane,
                                                  double& cx, double& cy) {
    const int t = base + lane;
    double dx = 0.0, dy = 0.0;
    if (t < L) {
        dx = (double)row[(int64_t)t * D];
        dy = (double)row[(int64_t)t * D + 1];
    }
    const double ix = wave_incl_scan(dx, lane), iy = wave_incl_scan(dy, lane);
    double px = __shfl_up(ix, 1, skr::kWave), py = __shfl_up(iy, 1, skr::kWave);
    if (lane == 0) px = py = 0.0;
    ChunkPoints p{cx + px, cy + py, cx + ix, cy + iy};
    cx += __shfl(ix, skr::kWave - 1, skr::kWave);
    cy += __shfl(iy, skr::kWave - 1, skr::kWave);
    return p;
}

__global__ __launch_bounds__(skr::kWave) void raster_geom(RasterArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int D = a.D, lift_col = a.D == 5 ? 3 : 2;
    int64_t len = a.lengths[b];
    const int L = (int)(len < 0 ? 0 : (len > a.N ? a.N : len));
    const float* row = a.strokes + (int64_t)b * a.N * D;
    float fs, fx, fy;
    if (a.frame_in) {
        fs = a.frame_in[b * 3], fx = a.frame_in[b * 3 + 1], fy = a.frame_in[b * 3 + 2];
    } else {
        // bounding box over P_0 .. P_L (the origin included)
        double cx = 0.0, cy = 0.0, x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;
        for (int base = 0; base < L; base += skr::kWave) {
            const ChunkPoints p = scan_chunk(row, D, base, L, lane, cx, cy);
            x0 = fmin(x0, p.ex), x1 = fmax(x1, p.ex);
            y0 = fmin(y0, p.ey), y1 = fmax(y1, p.ey);
        }
        x0 = wave_min(x0), x1 = wave_max(x1), y0 = wave_min(y0), y1 = wave_max(y1);
        const double e = fmax(x1 - x0, y1 - y0), half = 0.5 * (double)a.S;
        const double sc = e > 0.0 ? ((double)a.S - 2.0 * (double)a.pad) / e : 1.0;
        fs = (float)sc;
        fx = (float)(half - sc * (0.5 * (x0 + x1)));
        fy = (float)(half - sc * (0.5 * (y0 + y1)));
    }
    if (lane == 0) a.frame[b * 3] = fs, a.frame[b * 3 + 1] = fx, a.frame[b * 3 + 2] = fy;
    const double sc = (double)fs, ox = (double)fx, oy = (double)fy;
    float4* seg = reinterpret_cast<float4*>(a.seg) + (int64_t)b * a.N;
    double cx = 0.0, cy = 0.0;
    int cnt = 0;
    for (int base = 0; base < L; base += skr::kWave) {
        const ChunkPoints p = scan_chunk(row, D, base, L, lane, cx, cy);
        const int t = base + lane;
        const bool drawn = t >= 1 && t < L && row[(int64_t)(t - 1) * D + lift_col] < 0.5f;
        const unsigned long long m = __ballot(drawn);
        if (drawn) {
            const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
            seg[pos] = make_float4((float)(sc * p.sx + ox), (float)(sc * p.sy + oy),
                                   (float)(sc * p.ex + ox), (float)(sc * p.ey + oy));
        }
        cnt += __popcll(m);
    }
    if (lane == 0) a.count[b] = cnt;
}

__global__ __launch_bounds__(kThreads) void raster_tile(RasterArgs a) {
    __shared__ float4 s_seg[kChunk];   // (ax, ay, bx - ax, by - ay)
    __shared__ float s_inv[kChunk];    // 1 / |b - a|^2, 0 for a dot
    __shared__ int s_wcnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ntx = (a.S + kTile - 1) / kTile;
    const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
    const int b = a.b0 + blockIdx.y;
    const int px = tx * kTile + (tid & (kTile - 1)), py = ty * kTile + (tid / kTile);
    const float x = (float)px + 0.5f, y = (float)py + 0.5f;
    const float r = a.width * 0.5f + 0.5f;
    // the tile's pixel centres span [cx0, cx1] x [cy0, cy1]
    const float cx0 = (float)(tx * kTile) + 0.5f, cx1 = (float)min(tx * kTile + kTile, a.S) - 0.5f;
    const float cy0 = (float)(ty * kTile) + 0.5f, cy1 = (float)min(ty * kTile + kTile, a.S) - 0.5f;
    const int cnt = __builtin_amdgcn_readfirstlane(a.count[b]);
    const float4* seg = reinterpret_cast<const float4*>(a.seg) + (int64_t)b * a.N;
    float best = INFINITY;
    for (int base = 0; base < cnt; base += kChunk) {
        const int end = min(base + kChunk, cnt);
        int ns = 0;
        for (int r0 = base; r0 < end; r0 += kThreads) {
            const int i = r0 + tid;
            bool keep = false;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < end) {
                s = seg[i];
                // Distance from the segment's bounding box to the rectangle of pixel
                // centres. Past r no pixel of the tile gets ink from it; the slack
                // covers the rounding of the per-pixel distance, so that a dropped
                // segment's computed ink is exactly 0 too.
                const float gx = fmaxf(0.f, fmaxf(fminf(s.x, s.z) - cx1, cx0 - fmaxf(s.x, s.z)));
                const float gy = fmaxf(0.f, fmaxf(fminf(s.y, s.w) - cy1, cy0 - fmaxf(s.y, s.w)));
                const float big = fmaxf(fmaxf(fabsf(s.x), fabsf(s.z)), fmaxf(fabsf(s.y), fabsf(s.w)));
                const float thr = r + 0.01f + 1e-5f * big;
                keep = !a.cull || !(gx * gx + gy * gy > thr * thr);
            }
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_wcnt[w] = __popcll(m);
            __syncthreads();
            int off = ns, tot = 0;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) {
                const int c = s_wcnt[k];
                off += k < w ? c : 0;
                tot += c;
            }
            if (keep) {
                off += __popcll(m & ((1ull << lane) - 1ull));
                const float ux = s.z - s.x, uy = s.w - s.y, l2 = ux * ux + uy * uy;
                s_seg[off] = make_float4(s.x, s.y, ux, uy);
                s_inv[off] = l2 > 0.f ? 1.0f / l2 : 0.f;
            }
            ns += tot;
            __syncthreads();
        }
        // Every fused multiply-add is written out (contraction is off in this file):
        // left to the compiler, the copies of an unrolled loop contract differently,
        // and a pixel-segment distance would depend on the segment's place in the list.
        for (int k = 0; k < ns; ++k) {
            const float4 s = s_seg[k];
            const float vx = x - s.x, vy = y - s.y;
            const float t = fminf(fmaxf(fmaf(vx, s.z, vy * s.w) * s_inv[k], 0.f), 1.f);
            const float qx = fmaf(-t, s.z, vx), qy = fmaf(-t, s.w, vy);
            best = fminf(best, fmaf(qx, qx, qy * qy));
        }
        __syncthreads();
    }
    if (px < a.S && py < a.S)
        a.out[((int64_t)b * a.S + py) * a.S + px] = fminf(fmaxf(r - sqrtf(best), 0.f), 1.f);
}

}  // namespace

SKR_API int skr_raster(const RasterArgs* a, hipStream_t s) {
    if (a->B < 0 || a->N < 0 || (a->D != 3 && a->D != 5) || a->S < 1 || a->S > kMaxS) return -2;
    if (!(a->width > 0.f) || !(a->pad >= 0.f) || !(2.f * a->pad < (float)a->S)) return -3;
    if (a->B == 0) return 0;
    if (!a->lengths || !a->frame || !a->count || !a->out || (a->N > 0 && (!a->strokes || !a->seg)) ||
        ((uintptr_t)a->seg & 15))
        return -4;
    hipLaunchKernelGGL(raster_geom, dim3(a->B), dim3(skr::kWave), 0, s, *a);
    const int nt = (a->S + kTile - 1) / kTile;
    for (int b0 = 0; b0 < a->B; b0 += kMaxGridY) {
        RasterArgs t = *a;
        t.b0 = b0;
        const int nb = a->B - b0 < kMaxGridY ? a->B - b0 : kMaxGridY;
        hipLaunchKernelGGL(raster_tile, dim3(nt * nt, nb), dim3(kThreads), 0, s, t);
    }
    return SKR_CHECK_LAUNCH();
}

SKR_API int skr_raster_args_size() { return (int)sizeof(RasterArgs); }
