// sample_select.h -- the two workgroup steps the samplers share (cloud_sample.hip, volume_sample.hip): one round's digit pick of the 8-bit
// radix select, and the copy of rows staged in LDS to the outputs.  Both are written for a workgroup of 256 threads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wave_ops.h"

namespace ps {

// One round of the select, thread = digit: reads and clears the 256 bins of `hist` and finds the digit whose bucket holds the remaining
// rank.  s_need / s_rank are LDS words thread 0 has written before the call (how many are taken, the 0-based rank left); the barrier in
// here publishes them.  Nothing is picked when *s_need is 0.  Returns true in the one thread whose digit it is: that thread has or-ed
// the digit into *prefix at `shift` and gets the rank left inside the digit's bucket in `left`, for the caller to store.
__device__ __forceinline__ bool select_pick_digit(unsigned* hist, int shift, const unsigned* s_need, const unsigned* s_rank, unsigned* prefix,
                                                  unsigned& left)
{
    __shared__ unsigned s_w[4];
    const int d = threadIdx.x, lane = d & 63, wave = d >> 6;
    const unsigned c = hist[d];
    hist[d] = 0;
    const unsigned inc = wave_inclusive_sum(c, lane);
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    if (*s_need == 0) return false;
    unsigned below = inc - c;
    for (int w = 0; w < wave; ++w) below += s_w[w];
    const unsigned r = *s_rank;
    if (c && below <= r && r < below + c) {  // exactly one digit
        *prefix |= (unsigned)d << shift;
        left = r - below;
        return true;
    }
    return false;
}

// `count` 32-bit words staged in LDS (src 16-byte aligned) -> dst, by all threads of the workgroup; vec: dst is 16-byte aligned, use
// 16-byte stores
__device__ __forceinline__ void store_staged_words(const void* src_v, void* dst_v, unsigned count, bool vec)
{
    const uint32_t* src = static_cast<const uint32_t*>(src_v);
    uint32_t* dst = static_cast<uint32_t*>(dst_v);
    if (vec) {
        const unsigned n4 = count / 4;
        for (unsigned k = threadIdx.x; k < n4; k += 256) reinterpret_cast<uint4*>(dst)[k] = reinterpret_cast<const uint4*>(src)[k];
        for (unsigned k = n4 * 4 + threadIdx.x; k < count; k += 256) dst[k] = src[k];
    } else {
        for (unsigned k = threadIdx.x; k < count; k += 256) dst[k] = src[k];
    }
}
__device__ __forceinline__ void store_staged_words(const void* src, void* dst, unsigned count)
{
    store_staged_words(src, dst, count, (reinterpret_cast<uintptr_t>(dst) & 15) == 0);
}

}  // namespace ps
