// sample_hash.h -- the one definition of the hashes behind the samplers' rules (cloud_sample.hip: ps_cloud_sample; volume_sample.hip:
// ps_volume_sample), as include/pointseg.h states them and tests/cloud_sample_ref.py restates them.  All arithmetic is mod 2^32.
#pragma once
#include <hip/hip_runtime.h>

namespace ps {

constexpr unsigned kSeedMul = 0x9E3779B9u;   // s_sel(b) = hash32(seed + kSeedMul * (2b + 1)), s_perm(b) = hash32(seed + kSeedMul * (2b + 2))
constexpr unsigned kIndexMul = 2654435761u;  // key(i) = hash32(i * kIndexMul ^ s) << 32 | i

__host__ __device__ __forceinline__ unsigned hash32(unsigned x)  // lowbias32, as ops_train.hip's dropout
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// a bijection of i for every s (odd multiplier, xor, invertible mixer): no two points of a cloud share a hash
__host__ __device__ __forceinline__ unsigned point_hash(unsigned i, unsigned s) { return hash32(i * kIndexMul ^ s); }

}  // namespace ps
