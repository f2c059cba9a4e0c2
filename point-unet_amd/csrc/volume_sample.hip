// volume_sample.hip -- a CT volume and its positive set (a label, a mask, or an attention map turned into one) -> the network's clouds,
// on the device behind one call: the Pancreas preparation of PointSegment/utils/dataPreparePancreas.py:34-46, 132-169 (population z-score
// of ALL voxels; every positive voxel first and in voxel order, then a uniform sample of the rest, NOT shuffled), utils/genBinaryMap.py:67-80
// (probability >= threshold) and PointSegment/utils/over_sampling.py:58-65 (binary dilation OR truth), as the rule include/pointseg.h states
// for ps_volume_sample (restated in numpy by tests/volume_sample_ref.py).
//
// Nothing per voxel is ever stored but ONE byte of mask: the normalised volume, the coordinates, the keys and the background's index list
// do not exist; a voxel's selection hash is recomputed in every pass (sample_hash.h), as cloud_sample.hip does for a cloud's points.
//   1. statistics  one pass over the volume; int16: exact integer sums, n * sum(x^2) - sum(x)^2 formed in 128 bits (independent of the
//                  reduction order); float32: float64 sums of x - x[0] in one fixed order.  {mean, std} stay on the device for the gather.
//   2. mask        threshold / mask -> bytes; one pass per dilation round IN PLACE: round r reads bit (r & 1) of its six neighbours and
//                  writes bit ((r + 1) & 1) of its own bytes, keeping the bit the round reads, so a neighbour's concurrent read sees the
//                  same value before and after the store; the last pass ORs the truth in, leaves 0 / 1 and counts the positives (P).
//   3. select      four rounds of an 8-bit radix select of the threshold hash h*(l) of every loop l; ONE read of the mask serves all loops
//                  (a lane holds 16 voxels and updates `loops` LDS histograms; one global atomic per non-zero bin per workgroup).
//                  hash32(v * 2654435761 ^ s) is a bijection of v, so exactly N - P background voxels have hash <= h*(l).
//   4. compact     positives and, per loop, the background voxels with hash <= h*(l), appended through one cursor per loop (one
//                  returning atomic per workgroup and 16 384 voxels) as (key, v) pairs: key = l << 33 | v for a positive,
//                  l << 33 | 1 << 32 | hash for a background voxel.  The keys are unique, so the order of arrival does not matter:
//   5. sort        LSD radix sort of the loops * N pairs (sortscan.hip) = positives ascending, then ascending (hash, v), loop after loop.
//   6. gather      per output row: v -> (x, y, z), the raw voxel, label; xyz / origin rows staged in LDS and written with 16-byte stores.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "sample_hash.h"
#include "sample_select.h"
#include "sortscan.h"

namespace ps {

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;                                // voxels per lane and 16-byte load of the mask
constexpr unsigned kTile = kThreads * kPerThread;             // voxels per workgroup step of the per-voxel passes
constexpr int kChunks = 4;
constexpr unsigned kSuper = kTile * kChunks;                  // voxels per cursor reservation of the compaction
constexpr int kMaxLoops = PS_VOLUME_SAMPLE_MAX_LOOPS;
constexpr int kStatBlocks = 1024;                             // workgroups (= partials) of the statistics pass
constexpr unsigned kGrid = 2048;                              // workgroups of the select / compaction passes (grid-stride over tiles)

struct VsSeeds { unsigned s[kMaxLoops]; };  // s_sel(l), a kernel argument

// device state of one call (zeroed by a memset in front of the kernels)
struct VsState {
    unsigned hist[kMaxLoops][256];
    unsigned prefix[kMaxLoops];  // selection-hash bits found so far; h*(l) after round 3
    unsigned rank[kMaxLoops];    // 0-based rank left inside the bucket of `prefix`
    unsigned cursor[kMaxLoops];  // background rows appended so far
    unsigned positives;          // P, counted by the last mask pass
    unsigned need;               // N - P (0 when P > N: only the first N positives to arrive are written)
    unsigned pos_cursor;
    unsigned pad;
    int status[4];               // {P > N, P, N, 0}
    double stats[2];             // {mean, std}
};

union Bytes16 {
    uint4 q;
    uint8_t b[16];
};

// 16 bytes of a caller's u8 volume at voxel v0 (a multiple of 16), zeros from voxel n on; one 16-byte load where the pointer allows
__device__ __forceinline__ Bytes16 load16_u8(const uint8_t* __restrict__ p, unsigned v0, unsigned n, bool aligned)
{
    Bytes16 r;
    if (aligned && v0 + 16u <= n) {
        r.q = *reinterpret_cast<const uint4*>(p + v0);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) r.b[j] = v0 + j < n ? p[v0 + j] : (uint8_t)0;
    }
    return r;
}

__device__ __forceinline__ void store16_u8(uint8_t* __restrict__ p, unsigned v0, unsigned n, bool aligned, const Bytes16& r)
{
    if (aligned && v0 + 16u <= n) {
        *reinterpret_cast<uint4*>(p + v0) = r.q;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (v0 + j < n) p[v0 + j] = r.b[j];
    }
}

// fixed-order tree over the 256 threads of a workgroup (the same order every run: float64 sums are reproducible)
template <class A, class B>
__device__ __forceinline__ void block_sum2(A& a, B& b, A* sa, B* sb)
{
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sa[threadIdx.x] += sa[threadIdx.x + o];
            sb[threadIdx.x] += sb[threadIdx.x + o];
        }
        __syncthreads();
    }
    a = sa[0];
    b = sb[0];
}

// ---- 1. statistics ----------------------------------------------------------------------------------------------------------------------

// int16: part[block] = sum x, part[blocks + block] = sum x^2 (|sum x| < 2^46, sum x^2 <= 2^61: exact)
__global__ __launch_bounds__(256) void vs_stats_i16_kernel(const int16_t* __restrict__ vol, unsigned n, long long* __restrict__ part)
{
    __shared__ long long sa[256];
    __shared__ unsigned long long sb[256];
    long long s = 0;
    unsigned long long q = 0;
    const unsigned gid = blockIdx.x * 256u + threadIdx.x, gsz = gridDim.x * 256u;
    unsigned done = 0;
    if ((reinterpret_cast<uintptr_t>(vol) & 15) == 0) {  // eight voxels per 16-byte load
        const unsigned n8 = n / 8;
        for (unsigned c = gid; c < n8; c += gsz) {
            const int4 w = reinterpret_cast<const int4*>(vol)[c];
            const int ws[4] = {w.x, w.y, w.z, w.w};
            int ls = 0;
            unsigned long long lq = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int lo = (int)(short)(ws[k] & 0xffff), hi = ws[k] >> 16;
                ls += lo + hi;
                lq += (unsigned)(lo * lo) + (unsigned)(hi * hi);  // <= 2^31
            }
            s += ls;
            q += lq;
        }
        done = n8 * 8;
    }
    for (unsigned i = done + gid; i < n; i += gsz) {
        const int x = vol[i];
        s += x;
        q += (unsigned)(x * x);
    }
    block_sum2(s, q, sa, sb);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        part[gridDim.x + blockIdx.x] = (long long)q;
    }
}

// float32: part[block] = sum d, part[blocks + block] = sum d^2 with d = (double)x - (double)x[0] (the shift keeps the cancellation of
// sum d^2 - (sum d)^2 / n small when |mean| >> std; the variance does not depend on it)
__global__ __launch_bounds__(256) void vs_stats_f32_kernel(const float* __restrict__ vol, unsigned n, double* __restrict__ part)
{
    __shared__ double sa[256];
    __shared__ double sb[256];
    const double pivot = (double)vol[0];
    double s = 0.0, q = 0.0;
    const unsigned gid = blockIdx.x * 256u + threadIdx.x, gsz = gridDim.x * 256u;
    unsigned done = 0;
    if ((reinterpret_cast<uintptr_t>(vol) & 15) == 0) {
        const unsigned n4 = n / 4;
        for (unsigned c = gid; c < n4; c += gsz) {
            const float4 w = reinterpret_cast<const float4*>(vol)[c];
            const double d0 = (double)w.x - pivot, d1 = (double)w.y - pivot, d2 = (double)w.z - pivot, d3 = (double)w.w - pivot;
            s += (d0 + d1) + (d2 + d3);
            q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
        done = n4 * 4;
    }
    for (unsigned i = done + gid; i < n; i += gsz) {
        const double d = (double)vol[i] - pivot;
        s += d;
        q += d * d;
    }
    block_sum2(s, q, sa, sb);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s;
        part[gridDim.x + blockIdx.x] = q;
    }
}

// a 128-bit unsigned integer rounded ONCE to float64 (round to nearest even: the 64 leading bits with a sticky bit, converted by the
// hardware, then scaled by a power of two)
__device__ __forceinline__ double u128_to_double(unsigned long long hi, unsigned long long lo)
{
    if (hi == 0) return (double)lo;
    const int sh = __clzll((long long)hi);
    unsigned long long top = sh ? (hi << sh) | (lo >> (64 - sh)) : hi;
    const unsigned long long rest = sh ? lo << sh : lo;
    if (rest) top |= 1ull;  // bit 0 lies below the 53 kept bits and the rounding bit
    return ldexp((double)top, 64 - sh);
}

// one workgroup: the partials -> {mean, std} (state and, if asked for, the caller's out_stats); also publishes P
template <bool INT>
__global__ __launch_bounds__(256) void vs_stats_finish_kernel(const void* __restrict__ part_v, int nb, unsigned n, const float* __restrict__ vol_f32,
                                                              VsState* __restrict__ st, double* __restrict__ out_stats, bool have_stats,
                                                              long long* __restrict__ out_positives)
{
    __shared__ long long sa_i[256];
    __shared__ unsigned long long sb_i[256];
    __shared__ double sa_d[256];
    __shared__ double sb_d[256];
    if (threadIdx.x == 0 && out_positives) out_positives[0] = (long long)st->positives;
    if (!have_stats) return;
    double mean, sd;
    if (INT) {
        const long long* part = static_cast<const long long*>(part_v);
        long long s = 0;
        unsigned long long q = 0;
        for (int b = threadIdx.x; b < nb; b += 256) {
            s += part[b];
            q += (unsigned long long)part[nb + b];
        }
        block_sum2(s, q, sa_i, sb_i);
        // n * Q - S^2 >= 0 (Cauchy-Schwarz), both products below 2^92
        const unsigned long long nn = n, as = (unsigned long long)(s < 0 ? -s : s);
        const unsigned long long a_lo = nn * q, a_hi = __umul64hi(nn, q), b_lo = as * as, b_hi = __umul64hi(as, as);
        const unsigned long long d_lo = a_lo - b_lo, d_hi = a_hi - b_hi - (a_lo < b_lo ? 1ull : 0ull);
        mean = (double)s / (double)n;
        sd = sqrt(u128_to_double(d_hi, d_lo)) / (double)n;
    } else {
        const double* part = static_cast<const double*>(part_v);
        double s = 0.0, q = 0.0;
        for (int b = threadIdx.x; b < nb; b += 256) {
            s += part[b];
            q += part[nb + b];
        }
        block_sum2(s, q, sa_d, sb_d);
        const double m = s / (double)n;
        double var = (q - s * m) / (double)n;
        if (var < 0.0) var = 0.0;
        mean = (double)vol_f32[0] + m;
        sd = sqrt(var);
    }
    if (threadIdx.x == 0) {
        st->stats[0] = mean;
        st->stats[1] = sd;
        if (out_stats) {
            out_stats[0] = mean;
            out_stats[1] = sd;
        }
    }
}

// ---- 2. mask ----------------------------------------------------------------------------------------------------------------------------

// SRC 0: the caller's u8 mask (!= 0); 1: probs[v, ch] >= thr in float32; 2: bit `rbit` of the work bytes (after the dilation).
// FIN: OR the truth in, write 0 / 1 (work bytes and out_mask) and count the positives; otherwise bit 0 of the work bytes for round 0.
template <int SRC, bool FIN>
__global__ __launch_bounds__(256) void vs_mask_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ probs, int C, int ch, float thr,
                                                      int rbit, const uint8_t* __restrict__ truth, uint8_t* m, uint8_t* __restrict__ out_mask,
                                                      unsigned n, VsState* __restrict__ st)
{
    __shared__ unsigned s_cnt[4];
    __shared__ __attribute__((aligned(16))) uint8_t s_flag[SRC == 1 ? kTile : 16];
    const unsigned v0 = (blockIdx.x * 256u + threadIdx.x) * 16u;
    unsigned cnt = 0;
    if (SRC == 1) {
        // the workgroup's 4096 x C floats are one contiguous run: consecutive lanes read consecutive 16 bytes (a lane's own 16 voxels lie
        // 64 C bytes from its neighbour's), the compared channel lands as one flag byte per voxel in LDS
        const unsigned tile0 = blockIdx.x * kTile;
        const unsigned count = (n - tile0 < kTile ? n - tile0 : kTile) * (unsigned)C;  // floats of this tile
        const float* src = probs + (size_t)tile0 * C;
        auto put = [&](unsigned f, float x) {
            const unsigned vox = C == 2 ? f >> 1 : f / (unsigned)C;
            if (f - vox * (unsigned)C == (unsigned)ch) s_flag[vox] = (uint8_t)(x >= thr);
        };
        if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            const unsigned n4 = count / 4;
            for (unsigned k = threadIdx.x; k < n4; k += 256) {
                const float4 w = reinterpret_cast<const float4*>(src)[k];
                put(4 * k, w.x);
                put(4 * k + 1, w.y);
                put(4 * k + 2, w.z);
                put(4 * k + 3, w.w);
            }
            for (unsigned f = n4 * 4 + threadIdx.x; f < count; f += 256) put(f, src[f]);
        } else {
            for (unsigned f = threadIdx.x; f < count; f += 256) put(f, src[f]);
        }
        __syncthreads();
    }
    if (v0 < n) {
        Bytes16 r;
        if (SRC == 0) {
            r = load16_u8(mask, v0, n, (reinterpret_cast<uintptr_t>(mask) & 15) == 0);
#pragma unroll
            for (int j = 0; j < 16; ++j) r.b[j] = r.b[j] != 0;
        } else if (SRC == 1) {
            r.q = *reinterpret_cast<const uint4*>(s_flag + threadIdx.x * 16u);
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (v0 + j >= n) r.b[j] = 0;
        } else {
            r.q = *reinterpret_cast<const uint4*>(m + v0);
#pragma unroll
            for (int j = 0; j < 16; ++j) r.b[j] = (r.b[j] >> rbit) & 1;
        }
        if (FIN) {
            if (truth) {
                const Bytes16 t = load16_u8(truth, v0, n, (reinterpret_cast<uintptr_t>(truth) & 15) == 0);
#pragma unroll
                for (int j = 0; j < 16; ++j) r.b[j] |= (uint8_t)(t.b[j] != 0);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) cnt += r.b[j];
            if (out_mask) store16_u8(out_mask, v0, n, (reinterpret_cast<uintptr_t>(out_mask) & 15) == 0, r);
        }
        *reinterpret_cast<uint4*>(m + v0) = r.q;  // (the work bytes are padded to a multiple of 256 and 256-byte aligned; bytes from n on are 0)
    }
    if (FIN) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += (unsigned)__shfl_xor((int)cnt, o);
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            if (tot) atomicAdd(&st->positives, tot);
        }
    }
}

// the 16 work bytes at start .. start + 15 (any alignment), zeros outside [0, npad)
__device__ __forceinline__ Bytes16 load16_any(const uint8_t* m, long long start, long long npad)
{
    Bytes16 r;
    if (start >= 0 && start + 16 <= npad) {
        __builtin_memcpy(&r.q, m + start, 16);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) r.b[j] = (start + j >= 0 && start + j < npad) ? m[start + j] : (uint8_t)0;
    }
    return r;
}

// one round of scipy.ndimage.binary_dilation's default structure (the 6-neighbourhood; outside the array = 0), in place: reads bit
// `rbit`, writes bit `rbit ^ 1`, keeps bit `rbit` of every byte it stores.  A lane owns 16 consecutive voxels of the flat volume; its four
// y / x neighbour runs are the 16 bytes at v0 -+ Z and v0 -+ Y Z, valid per voxel by that voxel's own (x, y).
__global__ __launch_bounds__(256) void vs_dilate_kernel(uint8_t* m, unsigned n, unsigned npad, unsigned X, unsigned Y, unsigned Z, int rbit)
{
    const unsigned v0 = (blockIdx.x * 256u + threadIdx.x) * 16u;
    if (v0 >= n) return;
    const long long yz = (long long)Y * Z;
    Bytes16 own, out;
    own.q = *reinterpret_cast<const uint4*>(m + v0);
    const Bytes16 ym = load16_any(m, (long long)v0 - Z, npad), yp = load16_any(m, (long long)v0 + Z, npad);
    const Bytes16 xm = load16_any(m, (long long)v0 - yz, npad), xp = load16_any(m, (long long)v0 + yz, npad);
    const unsigned left = v0 ? m[v0 - 1] : 0u, right = v0 + 16u < npad ? m[v0 + 16] : 0u;
    unsigned z = v0 % Z, t = v0 / Z, y = t % Y, x = t / Y;
    if (z + 16u <= Z && v0 + 16u <= n) {
        // the 16 voxels lie in one z-row (every lane when Z is a multiple of 16): x and y are the lane's, only the two end voxels can sit on a
        // z face, and the round is word arithmetic on the four 32-bit words -- byte j's z-neighbours are the 128-bit value moved by one byte
        const unsigned w[4] = {own.q.x, own.q.y, own.q.z, own.q.w};
        const unsigned lo = z > 0 ? left & 255u : 0u, hi = z + 16u < Z ? right & 255u : 0u;
        const unsigned ymk = y > 0 ? ~0u : 0u, ypk = y + 1 < Y ? ~0u : 0u, xmk = x > 0 ? ~0u : 0u, xpk = x + 1 < X ? ~0u : 0u;
        const unsigned a[4] = {ym.q.x, ym.q.y, ym.q.z, ym.q.w}, b[4] = {yp.q.x, yp.q.y, yp.q.z, yp.q.w};
        const unsigned c[4] = {xm.q.x, xm.q.y, xm.q.z, xm.q.w}, e[4] = {xp.q.x, xp.q.y, xp.q.z, xp.q.w};
        const unsigned keep = 0x01010101u << rbit;
        unsigned o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned prev = (w[k] << 8) | (k ? w[k - 1] >> 24 : lo), next = (w[k] >> 8) | ((k < 3 ? w[k + 1] : hi) << 24);
            const unsigned d = w[k] | prev | next | (a[k] & ymk) | (b[k] & ypk) | (c[k] & xmk) | (e[k] & xpk);
            o[k] = (w[k] & keep) | (((d >> rbit) & 0x01010101u) << (rbit ^ 1));
        }
        *reinterpret_cast<uint4*>(m + v0) = make_uint4(o[0], o[1], o[2], o[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        unsigned o = 0;
        if (v0 + j < n) {
            const unsigned prev = j ? own.b[j - 1] : left, next = j < 15 ? own.b[j + 1] : right;
            unsigned d = own.b[j];
            if (z > 0) d |= prev;
            if (z + 1 < Z) d |= next;
            if (y > 0) d |= ym.b[j];
            if (y + 1 < Y) d |= yp.b[j];
            if (x > 0) d |= xm.b[j];
            if (x + 1 < X) d |= xp.b[j];
            o = (own.b[j] & (1u << rbit)) | (((d >> rbit) & 1u) << (rbit ^ 1));
        }
        out.b[j] = (uint8_t)o;
        if (++z == Z) {
            z = 0;
            if (++y == Y) {
                y = 0;
                ++x;
            }
        }
    }
    *reinterpret_cast<uint4*>(m + v0) = out.q;
}

// ---- 3. select --------------------------------------------------------------------------------------------------------------------------

// one round for every loop: histograms of digit (hash >> shift) & 255 over the background voxels whose higher digits equal the loop's prefix
__global__ __launch_bounds__(256) void vs_hist_kernel(const uint8_t* __restrict__ m, unsigned n, VsSeeds sd, int loops, VsState* __restrict__ st, int shift)
{
    __shared__ unsigned h[kMaxLoops * 256];
    __shared__ unsigned s_want[kMaxLoops];
    const bool first = shift == 24;
    if (!first && st->need == 0) return;  // nothing to select
    const unsigned hi_mask = first ? 0u : ~0u << (shift + 8);
    for (int i = threadIdx.x; i < loops * 256; i += 256) h[i] = 0;
    if ((int)threadIdx.x < loops) s_want[threadIdx.x] = first ? 0u : (st->prefix[threadIdx.x] & hi_mask);
    __syncthreads();
    for (unsigned long long t0 = (unsigned long long)blockIdx.x * kTile; t0 < n; t0 += (unsigned long long)gridDim.x * kTile) {
        const unsigned v0 = (unsigned)t0 + threadIdx.x * 16u;
        if (v0 >= n) continue;
        Bytes16 r;
        r.q = *reinterpret_cast<const uint4*>(m + v0);
#pragma unroll  // (fully: a run-time j would index the 16 bytes through scratch)
        for (int j = 0; j < 16; ++j) {
            const unsigned v = v0 + j;
            if (v >= n || r.b[j]) continue;
            const unsigned u = v * kIndexMul;
            for (int l = 0; l < loops; ++l) {
                const unsigned x = hash32(u ^ sd.s[l]);
                if ((x & hi_mask) == s_want[l]) atomicAdd(&h[l * 256 + ((x >> shift) & 255u)], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < loops * 256; i += 256)
        if (h[i]) atomicAdd(&st->hist[0][0] + i, h[i]);
}

// the digit whose bucket holds the remaining rank; clears the histogram for the next round.  Round 0 turns P into the number of background
// voxels to take and raises the status when P > N.  grid `loops`, 256 threads (thread = digit).
__global__ __launch_bounds__(256) void vs_pick_kernel(VsState* __restrict__ st, unsigned N, int shift)
{
    __shared__ unsigned s_need, s_rank;
    const int l = blockIdx.x;
    if (threadIdx.x == 0) {
        const unsigned P = st->positives;
        const unsigned need = P > N ? 0u : N - P;
        if (shift == 24) {
            st->rank[l] = need ? need - 1 : 0u;
            if (l == 0) {
                st->need = need;
                st->status[0] = P > N;
                st->status[1] = (int)P;
                st->status[2] = (int)N;
            }
        }
        s_need = need;
        s_rank = st->rank[l];
    }
    unsigned left;
    if (select_pick_digit(st->hist[l], shift, &s_need, &s_rank, &st->prefix[l], left)) st->rank[l] = left;
}

// ---- 4. compact -------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void vs_compact_kernel(const uint8_t* __restrict__ m, unsigned n, VsSeeds sd, int loops, unsigned N,
                                                         VsState* __restrict__ st, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals)
{
    __shared__ unsigned s_cnt[kMaxLoops + 1], s_base[kMaxLoops + 1];  // entry `loops`: the positives
    __shared__ unsigned s_thr[kMaxLoops];
    const unsigned P = st->positives;
    const bool draw = st->need != 0;
    if ((int)threadIdx.x < loops) s_thr[threadIdx.x] = st->prefix[threadIdx.x];
    for (unsigned long long b0 = (unsigned long long)blockIdx.x * kSuper; b0 < n; b0 += (unsigned long long)gridDim.x * kSuper) {
        if ((int)threadIdx.x <= loops) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        // bit c * 16 + j of the masks below: voxel b0 + c * kTile + threadIdx.x * 16 + j
        unsigned long long pm = 0, bg = 0;
#pragma unroll
        for (int c = 0; c < kChunks; ++c) {
            const unsigned long long vc = b0 + (unsigned long long)c * kTile + threadIdx.x * 16u;
            if (vc >= n) continue;
            Bytes16 r;
            r.q = *reinterpret_cast<const uint4*>(m + vc);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (vc + j >= n) continue;
                if (r.b[j]) pm |= 1ull << (c * 16 + j);
                else bg |= 1ull << (c * 16 + j);
            }
        }
        auto voxel = [&](int bit) { return (unsigned)b0 + (unsigned)(bit >> 4) * kTile + threadIdx.x * 16u + (unsigned)(bit & 15); };
        const unsigned np = (unsigned)__popcll(pm);
        const unsigned lp = np ? atomicAdd(&s_cnt[loops], np) : 0u;
        unsigned long long sel[kMaxLoops];
        unsigned lb[kMaxLoops];
#pragma unroll
        for (int l = 0; l < kMaxLoops; ++l) {
            sel[l] = 0;
            lb[l] = 0;
            if (l < loops && draw) {
                const unsigned thr = s_thr[l], s = sd.s[l];
                for (unsigned long long rest = bg; rest; rest &= rest - 1) {
                    const int bit = __ffsll((long long)rest) - 1;
                    if (point_hash(voxel(bit), s) <= thr) sel[l] |= 1ull << bit;
                }
                if (sel[l]) lb[l] = atomicAdd(&s_cnt[l], (unsigned)__popcll(sel[l]));
            }
        }
        __syncthreads();
        if ((int)threadIdx.x <= loops && s_cnt[threadIdx.x])
            s_base[threadIdx.x] = atomicAdd((int)threadIdx.x == loops ? &st->pos_cursor : &st->cursor[threadIdx.x], s_cnt[threadIdx.x]);
        __syncthreads();
        if (pm) {  // a positive is a row of every loop
            unsigned r = s_base[loops] + lp;
            for (unsigned long long rest = pm; rest; rest &= rest - 1, ++r) {
                const unsigned v = voxel(__ffsll((long long)rest) - 1);
                if (r < N)
                    for (int l = 0; l < loops; ++l) {
                        keys[(size_t)l * N + r] = (unsigned long long)l << 33 | v;
                        vals[(size_t)l * N + r] = v;
                    }
            }
        }
#pragma unroll
        for (int l = 0; l < kMaxLoops; ++l) {
            if (sel[l] == 0) continue;
            unsigned r = P + s_base[l] + lb[l];
            for (unsigned long long rest = sel[l]; rest; rest &= rest - 1, ++r) {
                const unsigned v = voxel(__ffsll((long long)rest) - 1);
                if (r < N) {
                    keys[(size_t)l * N + r] = (unsigned long long)l << 33 | 1ull << 32 | point_hash(v, sd.s[l]);
                    vals[(size_t)l * N + r] = v;
                }
            }
        }
        __syncthreads();  // (s_cnt / s_base are reused by the next step)
    }
}

// ---- 6. gather --------------------------------------------------------------------------------------------------------------------------

// row t of the output (flat over [loops, N]).  The 12-byte rows of a workgroup are contiguous: staged in LDS, written with 16-byte stores
// (row t0 * 3 words is 16-byte aligned since t0 is a multiple of 256).
template <class T>
__global__ __launch_bounds__(256) void vs_gather_kernel(const T* __restrict__ vol, const uint8_t* __restrict__ m, const uint8_t* __restrict__ label_src,
                                                        const unsigned* __restrict__ vals, unsigned n, unsigned total, unsigned X, unsigned Y, unsigned Z,
                                                        const VsState* __restrict__ st, float* __restrict__ out_xyz, float* __restrict__ out_f,
                                                        int32_t* __restrict__ out_l, int32_t* __restrict__ out_o, int32_t* __restrict__ out_i)
{
    __shared__ __attribute__((aligned(16))) float s_x[256 * 3];
    __shared__ __attribute__((aligned(16))) int32_t s_o[256 * 3];
    const unsigned t0 = blockIdx.x * 256u, t = t0 + threadIdx.x;
    const unsigned rows = total - t0 < 256u ? total - t0 : 256u;
    if (t < total) {
        unsigned v = vals[t];
        if (v >= n) v = 0;  // (only after P > N, where rows were left unwritten: a guard against a read past the volume)
        const unsigned z = v % Z, q = v / Z, y = q % Y, x = q / Y;
        const float fx = (float)x / (float)X, fy = (float)y / (float)Y, fz = (float)z / (float)Z;
        s_x[3 * threadIdx.x] = fx;
        s_x[3 * threadIdx.x + 1] = fy;
        s_x[3 * threadIdx.x + 2] = fz;
        s_o[3 * threadIdx.x] = (int32_t)x;
        s_o[3 * threadIdx.x + 1] = (int32_t)y;
        s_o[3 * threadIdx.x + 2] = (int32_t)z;
        if (out_f) {
            const float value = (float)(((double)vol[v] - st->stats[0]) / st->stats[1]);
            if ((reinterpret_cast<uintptr_t>(out_f) & 15) == 0) {
                reinterpret_cast<float4*>(out_f)[t] = make_float4(fx, fy, fz, value);
            } else {
                out_f[4 * (size_t)t] = fx;
                out_f[4 * (size_t)t + 1] = fy;
                out_f[4 * (size_t)t + 2] = fz;
                out_f[4 * (size_t)t + 3] = value;
            }
        }
        if (out_l) out_l[t] = label_src ? (int32_t)label_src[v] : (int32_t)m[v];
        if (out_i) out_i[t] = (int32_t)v;
    }
    __syncthreads();
    if (out_xyz) store_staged_words(s_x, out_xyz + (size_t)t0 * 3, rows * 3);
    if (out_o) store_staged_words(s_o, out_o + (size_t)t0 * 3, rows * 3);
}

size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }

}  // namespace

}  // namespace ps

extern "C" int ps_volume_sample(ps_context* c, ps_volume_sample_args* a)
{
    using namespace ps;
    // every argument error is found here, before anything is enqueued
    PS_CHECK(c && a, "ps_volume_sample: NULL argument");
    PS_CHECK(a->X >= 1 && a->Y >= 1 && a->Z >= 1 && a->X <= 65535 && a->Y <= 65535 && a->Z <= 65535,
             "ps_volume_sample: volume %lld x %lld x %lld (every dimension must be in [1, 65535])", (long long)a->X, (long long)a->Y, (long long)a->Z);
    const int64_t n64 = a->X * a->Y * a->Z;
    PS_CHECK(n64 < (1ll << 31), "ps_volume_sample: %lld voxels, need X * Y * Z < 2^31", (long long)n64);
    const bool draw = a->N > 0;
    const bool want_stats = a->out_stats || (draw && a->out_features);
    PS_CHECK(a->volume || !want_stats, "ps_volume_sample: volume is NULL but out_stats / out_features need it");
    PS_CHECK(!a->volume || a->volume_dtype == PS_VOLUME_I16 || a->volume_dtype == PS_VOLUME_F32,
             "ps_volume_sample: volume_dtype = %d is neither PS_VOLUME_I16 nor PS_VOLUME_F32", (int)a->volume_dtype);
    PS_CHECK((a->mask != nullptr) != (a->probs != nullptr), "ps_volume_sample: exactly one of mask and probs gives the positive set");
    if (a->probs) {
        PS_CHECK(a->probs_C >= 1 && a->probs_C <= 65535 && a->probs_channel >= 0 && a->probs_channel < a->probs_C, "ps_volume_sample: probs_channel = %d of probs_C = %d",
                 (int)a->probs_channel, (int)a->probs_C);
        PS_CHECK(a->threshold == a->threshold, "ps_volume_sample: threshold is NaN");
    }
    PS_CHECK(a->dilate >= 0 && a->dilate <= PS_VOLUME_SAMPLE_MAX_DILATE, "ps_volume_sample: dilate = %d, must be in [0, %d]", (int)a->dilate,
             PS_VOLUME_SAMPLE_MAX_DILATE);
    PS_CHECK(a->N >= 0, "ps_volume_sample: N = %lld is negative", (long long)a->N);
    PS_CHECK(a->reserved == 0, "ps_volume_sample: reserved = %u, must be 0", (unsigned)a->reserved);
    if (draw) {
        PS_CHECK(a->loops >= 1 && a->loops <= PS_VOLUME_SAMPLE_MAX_LOOPS, "ps_volume_sample: loops = %d, must be in [1, %d]", (int)a->loops,
                 PS_VOLUME_SAMPLE_MAX_LOOPS);
        PS_CHECK(a->N <= n64, "ps_volume_sample: N = %lld is larger than the volume (%lld voxels)", (long long)a->N, (long long)n64);
        PS_CHECK((int64_t)a->loops * a->N < (1ll << 31), "ps_volume_sample: loops * N = %lld, need < 2^31", (long long)((int64_t)a->loops * a->N));
    }
    const unsigned n = (unsigned)n64, N = (unsigned)a->N;
    const int loops = draw ? a->loops : 0;
    const size_t total = (size_t)loops * N;
    const size_t sort_words = sort_workspace_words(total);
    // the scratch: work bytes of the mask | state | statistics partials | sort pairs (ping-pong) | sort workspace
    const size_t npad = pad256(n);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += pad256(bytes); return o; };
    const size_t o_mask = take(npad), o_state = take(sizeof(VsState)), o_part = take(sizeof(double) * 2 * kStatBlocks);
    const size_t o_k0 = take(8 * total), o_k1 = take(8 * total), o_v0 = take(4 * total), o_v1 = take(4 * total), o_work = take(4 * sort_words);
    if (!a->scratch) {  // the first call of the two-call protocol
        a->scratch_bytes = (int64_t)off;
        return PS_OK;
    }
    PS_CHECK(a->scratch_bytes >= (int64_t)off, "ps_volume_sample: scratch_bytes = %lld, this call needs %lld", (long long)a->scratch_bytes, (long long)off);
    PS_CHECK((reinterpret_cast<uintptr_t>(a->scratch) & 255) == 0, "ps_volume_sample: scratch must be 256-byte aligned");
    char* base = static_cast<char*>(a->scratch);
    uint8_t* m = reinterpret_cast<uint8_t*>(base + o_mask);
    VsState* st = reinterpret_cast<VsState*>(base + o_state);
    void* part = base + o_part;
    unsigned long long *k0 = reinterpret_cast<unsigned long long*>(base + o_k0), *k1 = reinterpret_cast<unsigned long long*>(base + o_k1);
    unsigned *v0 = reinterpret_cast<unsigned*>(base + o_v0), *v1 = reinterpret_cast<unsigned*>(base + o_v1), *work = reinterpret_cast<unsigned*>(base + o_work);
    VsSeeds sd = {};
    for (int l = 0; l < loops; ++l) sd.s[l] = hash32(a->seed + kSeedMul * (2u * l + 1u));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    const bool i16 = a->volume_dtype == PS_VOLUME_I16;
    {
        Stage stg(c, "volume_sample", 1);
        int launches = 0;
        PS_HIP(hipMemsetAsync(st, 0, sizeof(VsState), sm));
        PS_HIP(hipMemsetAsync(m + (npad - 256), 0, 256, sm));  // the bytes from n on stay 0 through every pass
        const int stat_blocks = (int)std::min<size_t>(kStatBlocks, ((size_t)n + 2047) / 2048);
        if (want_stats) {
            if (i16)
                hipLaunchKernelGGL(vs_stats_i16_kernel, dim3(stat_blocks), dim3(256), 0, sm, static_cast<const int16_t*>(a->volume), n,
                                   static_cast<long long*>(part));
            else
                hipLaunchKernelGGL(vs_stats_f32_kernel, dim3(stat_blocks), dim3(256), 0, sm, static_cast<const float*>(a->volume), n,
                                   static_cast<double*>(part));
            ++launches;
        }
        const dim3 vgrid((unsigned)(((size_t)n + kTile - 1) / kTile));
        const int rounds = a->dilate;
#define PS_VS_MASK(SRC, FIN, RBIT)                                                                                                              \
    hipLaunchKernelGGL((vs_mask_kernel<SRC, FIN>), vgrid, dim3(256), 0, sm, a->mask, a->probs, (int)a->probs_C, (int)a->probs_channel, a->threshold, \
                       RBIT, a->truth, m, a->out_mask, n, st)
        if (rounds == 0) {
            if (a->mask) PS_VS_MASK(0, true, 0);
            else PS_VS_MASK(1, true, 0);
            ++launches;
        } else {
            if (a->mask) PS_VS_MASK(0, false, 0);
            else PS_VS_MASK(1, false, 0);
            for (int r = 0; r < rounds; ++r)
                hipLaunchKernelGGL(vs_dilate_kernel, vgrid, dim3(256), 0, sm, m, n, (unsigned)npad, (unsigned)a->X, (unsigned)a->Y, (unsigned)a->Z, r & 1);
            PS_VS_MASK(2, true, rounds & 1);
            launches += 2 + rounds;
        }
#undef PS_VS_MASK
        if (i16)
            hipLaunchKernelGGL(vs_stats_finish_kernel<true>, dim3(1), dim3(256), 0, sm, part, stat_blocks, n, static_cast<const float*>(nullptr), st,
                               a->out_stats, want_stats, reinterpret_cast<long long*>(a->out_positives));
        else
            hipLaunchKernelGGL(vs_stats_finish_kernel<false>, dim3(1), dim3(256), 0, sm, part, stat_blocks, n, static_cast<const float*>(a->volume), st,
                               a->out_stats, want_stats, reinterpret_cast<long long*>(a->out_positives));
        ++launches;
        if (draw) {
            const dim3 sgrid((unsigned)std::min<size_t>(kGrid, ((size_t)n + kTile - 1) / kTile));
            for (int shift = 24; shift >= 0; shift -= 8) {
                hipLaunchKernelGGL(vs_hist_kernel, sgrid, dim3(256), 0, sm, m, n, sd, loops, st, shift);
                hipLaunchKernelGGL(vs_pick_kernel, dim3(loops), dim3(256), 0, sm, st, N, shift);
            }
            const dim3 cgrid((unsigned)std::min<size_t>(kGrid, ((size_t)n + kSuper - 1) / kSuper));
            hipLaunchKernelGGL(vs_compact_kernel, cgrid, dim3(256), 0, sm, m, n, sd, loops, N, st, k0, v0);
            int bits = 33;  // the loop above {background flag, 32-bit hash or voxel}
            while ((1 << (bits - 33)) < loops) ++bits;
            const int which = radix_sort_pairs_u64(sm, k0, k1, v0, v1, total, bits, work);
            const unsigned* sorted = which == 0 ? v0 : v1;
            const dim3 ggrid((unsigned)((total + 255) / 256));
            if (i16)
                hipLaunchKernelGGL(vs_gather_kernel<int16_t>, ggrid, dim3(256), 0, sm, static_cast<const int16_t*>(a->volume), m, a->label_src, sorted, n,
                                   (unsigned)total, (unsigned)a->X, (unsigned)a->Y, (unsigned)a->Z, st, a->out_xyz, a->out_features, a->out_labels,
                                   a->out_origin, a->out_idx);
            else
                hipLaunchKernelGGL(vs_gather_kernel<float>, ggrid, dim3(256), 0, sm, static_cast<const float*>(a->volume), m, a->label_src, sorted, n,
                                   (unsigned)total, (unsigned)a->X, (unsigned)a->Y, (unsigned)a->Z, st, a->out_xyz, a->out_features, a->out_labels,
                                   a->out_origin, a->out_idx);
            launches += 8 + 1 + radix_sort_pairs_launches(total, bits) + 1;
        }
        PS_HIP(hipGetLastError());
        stg.n = launches;
    }
    if (!draw) return PS_OK;
    // P > N is only known on the device
    if (c->deferred) return c->defer_status(st->status, 4 * sizeof(int), 2, c->volume_samples++);
    int32_t h_status[4] = {0, 0, 0, 0};
    PS_HIP(hipMemcpyAsync(h_status, st->status, sizeof h_status, hipMemcpyDeviceToHost, sm));
    PS_HIP(hipStreamSynchronize(sm));
    ++c->volume_samples;
    if (h_status[0]) {
        ps::set_error("ps_volume_sample: the positive set holds %d voxels, more than N = %d (nothing was written outside the outputs; their rows are "
                      "unspecified)", h_status[1], h_status[2]);
        return PS_ESTATE;
    }
    return PS_OK;
}
