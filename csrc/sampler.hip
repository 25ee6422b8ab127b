// On-device MDN sampler (reference capability R14, model.py:187-264).
//
// One wave per batch row. From the head output z [B, 3 + 6M] it draws a
// stroke (csrc/mdn_sample.h, shared with the fused decoder), then writes
// (a) the sampled stroke row into the output sequence and (b) the next
// decoder input -- so an N-step decode loop never returns to the host
// and can be captured whole in one HIP graph. Random numbers come from the
// same stateless hash as the dropout masks (seed read from device memory).
//
// mode 0 = reference: layout [dx, dy, eos, eoc, cont]; pi temperature only
//          from step 2 on; pen temperature ignored unless fix_pen; sigma not
//          scaled; a row stops after emitting eoc (done flag).
// mode 1 = sketch-rnn VAE: layout [dx, dy, p1, p2, p3]; temperature on pi and
//          pen from step 0; sigma scaled by the temperature; a row stops after
//          emitting p3.
// greedy: argmax component / pen, offset = mean.
//
// Sketch completion: the *_forced entry points take per-row given strokes;
// a row with step < nforced[b] emits forced[b] instead of its draw
// (mdn_sample.h: MdnForced, mdn_emit_row).
//
// Per-row temperature: the *_temps entry points take temps [B] (indexed by the
// launch's local row, like done and nforced); row b then uses temps[b] where
// the others use the scalar temp (mdn_sample.h: mdn_temp_gather).
#include "mdn_sample.h"

namespace {

__global__ __launch_bounds__(64) void mdn_sample_kernel(const float* __restrict__ z, int64_t ldz, int M, int mode,
                                                        float temp, int greedy, int fix_pen, const int64_t* seed,
                                                        uint32_t step, float* __restrict__ out_row, int64_t ld_out,
                                                        float* __restrict__ next_x, int64_t ld_next,
                                                        int* __restrict__ done, float* __restrict__ params,
                                                        const float* __restrict__ forced, int64_t ld_forced,
                                                        const int* __restrict__ nforced,
                                                        const float* __restrict__ temps, int row0,
                                                        const int* __restrict__ row_base) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float fv = skr::mdn_forced_load(forced, ld_forced, nforced, temps, b);
    const uint32_t key = skr::hash_key(*seed, 0x5A3Du, step);
    if (row_base != nullptr) row0 += *row_base;   // (a scalar load beside the seed's)
    const float tb = skr::mdn_temp_gather(fv, temps, temp);
    const skr::MdnDraw d =
        skr::mdn_sample_wave(z + b * ldz, M, mode, tb, 1.f / tb, greedy, fix_pen, key, (uint32_t)(row0 + b), step);
    const skr::MdnForced f = skr::mdn_forced_gather(fv);
    if (lane != 0) return;
    skr::mdn_emit_row(d, f, step, mode, out_row + b * ld_out, next_x + b * ld_next, done + b);
    if (params) {   // (of the draw, forced row or not)
        float* p = params + b * 4;
        p[0] = (float)d.idx;
        p[1] = (float)d.pidx;
        p[2] = d.s1;
        p[3] = d.s2;
    }
}

// Same, with z given as the sum of `nslab` split-K partial slabs of a head
// GEMM without bias (csrc/skinny_gemm.hip, z = h @ W_out in slabs) plus the
// bias. One 256-thread workgroup per row: wave w folds the slabs s = w mod 4
// of every column with independent (unrolled, clamped) loads, the four
// partial rows meet in LDS, then wave 0 samples.
__global__ __launch_bounds__(256) void mdn_sample_slabs_kernel(const float* __restrict__ zs, int64_t ldz, int nslab,
                                                               int64_t slab, const float* __restrict__ bias, int nout,
                                                               int M, int mode, float temp, int greedy, int fix_pen,
                                                               const int64_t* seed, uint32_t step, int row0,
                                                               float* __restrict__ out_row, int64_t ld_out,
                                                               float* __restrict__ next_x, int64_t ld_next,
                                                               int* __restrict__ done,
                                                               const float* __restrict__ forced, int64_t ld_forced,
                                                               const int* __restrict__ nforced,
                                                               const float* __restrict__ temps,
                                                               const int* __restrict__ row_base) {
    __shared__ float part[4][256];
    __shared__ float zrow[256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float fv = skr::mdn_forced_load(forced, ld_forced, nforced, temps, b);
    skr::fold_head_slabs(zs, ldz, nslab, slab, bias, nout, b, part, zrow);
    if (w != 0) return;
    const uint32_t key = skr::hash_key(*seed, 0x5A3Du, step);
    if (row_base != nullptr) row0 += *row_base;   // (a scalar load beside the seed's)
    const float tb = skr::mdn_temp_gather(fv, temps, temp);
    const skr::MdnDraw d = skr::mdn_sample_wave(zrow, M, mode, tb, 1.f / tb, greedy, fix_pen, key, (uint32_t)(row0 + b), step);
    const skr::MdnForced f = skr::mdn_forced_gather(fv);
    if (lane != 0) return;
    skr::mdn_emit_row(d, f, step, mode, out_row + b * ld_out, next_x + b * ld_next, done + b);
}

}  // namespace

// forced [B][ld_forced] / nforced [B] (indexed like `done`, by local row): rows
// with step < nforced[b] emit forced[b] instead of their draw (mdn_sample.h;
// every row of forced is read when nforced is given). temps [B] (local rows
// too): row b's temperature in place of temp; nullptr: temp for every row.
// row_base [1] (device memory, nullptr: 0): added to row0, so that a captured
// launch serves any block of a longer job list (GraphDecoder.run(row0=)).
SKR_API int skr_mdn_sample_slabs_rows(const float* zs, int64_t ldz, int nslab, int64_t slab, const float* bias, int B,
                                      int M, int mode, float temp, int greedy, int fix_pen, const int64_t* seed,
                                      uint32_t step, int row0, float* out_row, int64_t ld_out, float* next_x,
                                      int64_t ld_next, int* done, const float* forced, int64_t ld_forced,
                                      const int* nforced, const float* temps, const int* row_base, hipStream_t s) {
    if (M < 1 || M > 32 || nslab < 1) return -2;
    if (nforced != nullptr && forced == nullptr) return -2;
    if (B <= 0) return 0;
    hipLaunchKernelGGL(mdn_sample_slabs_kernel, dim3(B), dim3(256), 0, s, zs, ldz, nslab, slab, bias, 3 + 6 * M, M,
                       mode, temp, greedy, fix_pen, seed, step, row0, out_row, ld_out, next_x, ld_next, done, forced,
                       ld_forced, nforced, temps, row_base);
    return SKR_CHECK_LAUNCH();
}

SKR_API int skr_mdn_sample_slabs_temps(const float* zs, int64_t ldz, int nslab, int64_t slab, const float* bias, int B,
                                       int M, int mode, float temp, int greedy, int fix_pen, const int64_t* seed,
                                       uint32_t step, int row0, float* out_row, int64_t ld_out, float* next_x,
                                       int64_t ld_next, int* done, const float* forced, int64_t ld_forced,
                                       const int* nforced, const float* temps, hipStream_t s) {
    return skr_mdn_sample_slabs_rows(zs, ldz, nslab, slab, bias, B, M, mode, temp, greedy, fix_pen, seed, step, row0,
                                     out_row, ld_out, next_x, ld_next, done, forced, ld_forced, nforced, temps, nullptr,
                                     s);
}

SKR_API int skr_mdn_sample_slabs_forced(const float* zs, int64_t ldz, int nslab, int64_t slab, const float* bias, int B,
                                        int M, int mode, float temp, int greedy, int fix_pen, const int64_t* seed,
                                        uint32_t step, int row0, float* out_row, int64_t ld_out, float* next_x,
                                        int64_t ld_next, int* done, const float* forced, int64_t ld_forced,
                                        const int* nforced, hipStream_t s) {
    return skr_mdn_sample_slabs_temps(zs, ldz, nslab, slab, bias, B, M, mode, temp, greedy, fix_pen, seed, step, row0,
                                      out_row, ld_out, next_x, ld_next, done, forced, ld_forced, nforced, nullptr, s);
}

SKR_API int skr_mdn_sample_slabs(const float* zs, int64_t ldz, int nslab, int64_t slab, const float* bias, int B,
                                 int M, int mode, float temp, int greedy, int fix_pen, const int64_t* seed,
                                 uint32_t step, int row0, float* out_row, int64_t ld_out, float* next_x,
                                 int64_t ld_next, int* done, hipStream_t s) {
    return skr_mdn_sample_slabs_forced(zs, ldz, nslab, slab, bias, B, M, mode, temp, greedy, fix_pen, seed, step, row0,
                                       out_row, ld_out, next_x, ld_next, done, nullptr, 0, nullptr, s);
}

// row0 + *row_base (nullptr: 0): the hash row of local row 0 (a block of a
// larger job list keeps its rows' noise; done, nforced and temps stay indexed
// by the local row).
SKR_API int skr_mdn_sample_rows(const float* z, int64_t ldz, int B, int M, int mode, float temp, int greedy,
                                int fix_pen, const int64_t* seed, uint32_t step, int row0, float* out_row,
                                int64_t ld_out, float* next_x, int64_t ld_next, int* done, float* params,
                                const float* forced, int64_t ld_forced, const int* nforced, const float* temps,
                                const int* row_base, hipStream_t s) {
    if (M < 1 || M > 32) return -2;
    if (nforced != nullptr && forced == nullptr) return -2;
    if (B <= 0) return 0;
    hipLaunchKernelGGL(mdn_sample_kernel, dim3(B), dim3(64), 0, s, z, ldz, M, mode, temp, greedy, fix_pen, seed, step,
                       out_row, ld_out, next_x, ld_next, done, params, forced, ld_forced, nforced, temps, row0,
                       row_base);
    return SKR_CHECK_LAUNCH();
}

SKR_API int skr_mdn_sample_temps(const float* z, int64_t ldz, int B, int M, int mode, float temp, int greedy,
                                 int fix_pen, const int64_t* seed, uint32_t step, float* out_row, int64_t ld_out,
                                 float* next_x, int64_t ld_next, int* done, float* params, const float* forced,
                                 int64_t ld_forced, const int* nforced, const float* temps, hipStream_t s) {
    return skr_mdn_sample_rows(z, ldz, B, M, mode, temp, greedy, fix_pen, seed, step, 0, out_row, ld_out, next_x,
                               ld_next, done, params, forced, ld_forced, nforced, temps, nullptr, s);
}

SKR_API int skr_mdn_sample_forced(const float* z, int64_t ldz, int B, int M, int mode, float temp, int greedy,
                                  int fix_pen, const int64_t* seed, uint32_t step, float* out_row, int64_t ld_out,
                                  float* next_x, int64_t ld_next, int* done, float* params, const float* forced,
                                  int64_t ld_forced, const int* nforced, hipStream_t s) {
    return skr_mdn_sample_temps(z, ldz, B, M, mode, temp, greedy, fix_pen, seed, step, out_row, ld_out, next_x, ld_next,
                                done, params, forced, ld_forced, nforced, nullptr, s);
}

SKR_API int skr_mdn_sample(const float* z, int64_t ldz, int B, int M, int mode, float temp, int greedy, int fix_pen,
                           const int64_t* seed, uint32_t step, float* out_row, int64_t ld_out, float* next_x,
                           int64_t ld_next, int* done, float* params, hipStream_t s) {
    return skr_mdn_sample_forced(z, ldz, B, M, mode, temp, greedy, fix_pen, seed, step, out_row, ld_out, next_x,
                                 ld_next, done, params, nullptr, 0, nullptr, s);
}
