// Slot refill of the recycling bulk decoder (sample/stream.py).
//
// The four-launch HyperLSTM stroke (sample/hyper_step.py) keeps the state of
// `slots` rows in place. In bulk generation a row is a SLOT that works on
// one job (one latent) at a time; csrc/decode_step.hip's slot-map sampler
// sets done[slot] when the job's sketch ends. At the end of every replayed
// chunk of steps two small launches hand finished slots the next jobs:
//
//   1. refill_rank, ONE workgroup, one thread per slot: ranks the finished
//      slots in slot order (ballot + prefix sum over the waves), gives slot i
//      the job next + rank while jobs remain, and writes the assignment, the
//      new `next` and the word the host reads once per chunk: jobs not yet
//      handed out + slots that will be drawing in the next chunk.
//   2. refill_gather, one workgroup per slot: an assigned slot gets its job's
//      constants copied into the in-place state with 16-byte loads and
//      stores ([h0 | hh0] bf16, c0, hc0, the z-projection row, the
//      temperature) and its map reset (done = 0, pos = -1: a fresh slot); a
//      slot that is still drawing has pos advanced by the chunk length; a
//      finished slot without a job stays idle (done stays set, so nothing of
//      it is ever stored) -- with `poison` its state, z-projection and
//      stroke rows are NaN-filled, which must not change any result.
//
// `done` is the only criterion: the fused stroke draws stroke t inside step
// t + 1's launch, so a slot whose pending stroke will end it is picked up one
// chunk later. The first fill is the same pair with every slot marked done.
// No atomics: the assignment is a pure function of (done, next, jobs).
#include "common.h"

struct RefillArgs {
    int slots, chunk, poison;
    int* ctl;                 // [4] next job, jobs, the host's word, (unused)
    int* done;                // [slots]
    int* job;                 // [slots]
    int* pos;                 // [slots]
    int* assign;              // [slots] scratch: job (>= 0), -1 still drawing, -2 idle
    // in-place state rows (row strides in bytes, multiples of 16) and their per-job sources
    void* A; const void* jA; int a_bytes;          // [h | hh] bf16
    void* CC; const void* jCC; int cc_bytes;       // c fp32
    void* HCC; const void* jHCC; int hcc_bytes;    // hyper c fp32
    void* ZP; const void* jZP; int zp_bytes;       // z projections fp32
    float* temps; const float* jtemps;             // [slots] <- [jobs]
    float* X;                                      // [slots][5] (poison only)
};

namespace {

__global__ __launch_bounds__(1024) void refill_rank(const RefillArgs r) {
    __shared__ int wsum[16];
    const int i = threadIdx.x, lane = i & 63, w = i >> 6;
    const bool fin = i < r.slots && r.done[i] != 0;
    const unsigned long long m = __ballot(fin);
    if (i < 16) wsum[i] = 0;  // (the block has ceil(slots / 64) waves)
    __syncthreads();
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int c = wsum[k];
        before += k < w ? c : 0;
        total += c;
    }
    const int rank = before + __popcll(m & ((1ull << lane) - 1ull));
    const int next = r.ctl[0], jobs = r.ctl[1];
    const int left = max(jobs - next, 0);
    const int given = min(total, left);
    if (i < r.slots) r.assign[i] = !fin ? -1 : (rank < left ? next + rank : -2);
    __syncthreads();          // every thread has read ctl[0]
    if (i == 0) {
        r.ctl[0] = next + given;
        r.ctl[2] = (left - given) + (r.slots - total) + given;
    }
}

__device__ inline void copy16(void* dst, const void* src, int bytes) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    for (int k = threadIdx.x; k < bytes / 16; k += blockDim.x) d[k] = s[k];
}

__device__ inline void fill16(void* dst, uint32_t word, int bytes) {
    uint4* d = reinterpret_cast<uint4*>(dst);
    const uint4 v = make_uint4(word, word, word, word);
    for (int k = threadIdx.x; k < bytes / 16; k += blockDim.x) d[k] = v;
}

__global__ __launch_bounds__(256) void refill_gather(const RefillArgs r) {
    const int b = blockIdx.x;
    const int a = r.assign[b];
    char* A = (char*)r.A + (int64_t)b * r.a_bytes;
    char* CC = (char*)r.CC + (int64_t)b * r.cc_bytes;
    char* HCC = (char*)r.HCC + (int64_t)b * r.hcc_bytes;
    char* ZP = (char*)r.ZP + (int64_t)b * r.zp_bytes;
    if (a >= 0) {
        copy16(A, (const char*)r.jA + (int64_t)a * r.a_bytes, r.a_bytes);
        copy16(CC, (const char*)r.jCC + (int64_t)a * r.cc_bytes, r.cc_bytes);
        copy16(HCC, (const char*)r.jHCC + (int64_t)a * r.hcc_bytes, r.hcc_bytes);
        copy16(ZP, (const char*)r.jZP + (int64_t)a * r.zp_bytes, r.zp_bytes);
        if (threadIdx.x == 0) {
            r.temps[b] = r.jtemps[a];
            r.job[b] = a;
            r.pos[b] = -1;
            r.done[b] = 0;
        }
    } else if (a == -1) {
        if (threadIdx.x == 0) r.pos[b] += r.chunk;
    } else if (r.poison) {
        fill16(A, 0x7fc07fc0u, r.a_bytes);        // two bf16 NaNs
        fill16(CC, 0x7fc00000u, r.cc_bytes);
        fill16(HCC, 0x7fc00000u, r.hcc_bytes);
        fill16(ZP, 0x7fc00000u, r.zp_bytes);
        if (threadIdx.x < 5) r.X[b * 5 + threadIdx.x] = __int_as_float(0x7fc00000);
    }
}

}  // namespace

// r->slots in [1, 1024]; every *_bytes a positive multiple of 16 (rows and
// their per-job sources 16-byte aligned).
SKR_API int skr_decode_refill(const RefillArgs* r, hipStream_t st) {
    if (r->slots < 1 || r->slots > 1024 || r->chunk < 1) return -2;
    if (r->ctl == nullptr || r->done == nullptr || r->job == nullptr || r->pos == nullptr || r->assign == nullptr ||
        r->A == nullptr || r->CC == nullptr || r->HCC == nullptr || r->ZP == nullptr || r->temps == nullptr ||
        r->X == nullptr)
        return -3;
    const int bytes[4] = {r->a_bytes, r->cc_bytes, r->hcc_bytes, r->zp_bytes};
    for (int k = 0; k < 4; ++k)
        if (bytes[k] <= 0 || bytes[k] % 16) return -4;
    const uintptr_t ptrs[8] = {(uintptr_t)r->A,   (uintptr_t)r->jA,   (uintptr_t)r->CC, (uintptr_t)r->jCC,
                               (uintptr_t)r->HCC, (uintptr_t)r->jHCC, (uintptr_t)r->ZP, (uintptr_t)r->jZP};
    for (int k = 0; k < 8; ++k)
        if (ptrs[k] % 16) return -4;
    const int threads = (r->slots + 63) / 64 * 64;
    hipLaunchKernelGGL(refill_rank, dim3(1), dim3(threads), 0, st, *r);
    hipLaunchKernelGGL(refill_gather, dim3(r->slots), dim3(256), 0, st, *r);
    return SKR_CHECK_LAUNCH();
}

SKR_API int skr_decode_refill_size() { return (int)sizeof(RefillArgs); }
