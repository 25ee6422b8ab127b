// Store policy of a kernel's global outputs, chosen per output class at run
// time (skr_store_set_policy, csrc/skinny_gemm.hip) and compiled in as a
// template parameter of the storing epilogue.
//
//   ST_PLAIN  default-policy stores: the lines stay dirty in the storing
//             XCD's L2 until the end-of-kernel write-back.
//   ST_WT     write-through (sc1) stores: the bytes leave the L2 as they are
//             stored, so the launch ends with nothing to write back. Also
//             the form an in-launch hand-off needs (csrc/handoff.h), where it
//             is not a choice.
//
// Every policy stores the same bits.
#pragma once
#include "handoff.h"

namespace skr {

enum StorePolicy : int { ST_PLAIN = 0, ST_WT = 1, kStorePolicies = 2 };

// Output classes of the per-step launches (what reads the bytes, and when).
enum StoreClass : int {
    SC_SLAB = 0,   // split-K partial slabs the next launch sums (csrc/skinny_tile.h)
    SC_STEP = 1,   // step outputs the next launch reads: the modulation step's gate pre-activations
    SC_SAVE = 2,   // saves only the backward scan reads: the modulation vectors and the bf16 R
    kStoreClasses = 3
};

// 16 bytes per lane at byte offset `off` of the buffer `r` describes.
template <int ST>
__device__ __forceinline__ void st16(__amdgpu_buffer_rsrc_t r, uint32_t off, u32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(v, r, off, 0, ST == ST_WT ? kSc1 : 0);
}

// 8 bytes per lane.
template <int ST>
__device__ __forceinline__ void st8(__amdgpu_buffer_rsrc_t r, uint32_t off, unsigned int lo, unsigned int hi) {
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(u32x2{lo, hi}, r, off, 0, ST == ST_WT ? kSc1 : 0);
}

}  // namespace skr

// The policy in force for a class (host side; csrc/skinny_gemm.hip).
int skr_store_policy_of(int cls);
