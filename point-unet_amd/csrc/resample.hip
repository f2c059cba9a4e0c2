// resample.hip -- scipy.ndimage.zoom(x, zoom, order = 0 | 3) of a 3-D int16 / uint8 / float32 volume on the device, with the input flip
// and the output clip of the Pancreas CT resampling fused in: PointSegment/utils/cvt_CT_down.py:79-104 and cvt_CT.py:79-105, by the rule
// include/pointseg_prepare.h states for ps_volume_zoom (restated in numpy by tests/zoom_ref.py).  float64 on the vector ALUs throughout;
// no MFMA, no library: the work is a few streaming passes.
//
//   taps     one small launch: per output index of each axis the coordinate cc = j * ((n - 1) / (m - 1)) in double, then the four cubic
//            weights and mirrored tap indices (order 3) or the sample floor(cc + 0.5) (order 0); idx[0] = -1 marks cc > n - 1, the
//            output plane scipy zeroes.  Nothing is uploaded and no voxel recomputes a weight.
//   order 0  one gather through the three tables (also order 3 on integers when no axis changes its length).
//   order 3  axis after axis, shrinking axes first (no intermediate is larger than the input or the output): prefilter along the axis, then
//            the 4-tap interpolation along it into the other scratch buffer -- the filter of a later axis commutes with it.  The first
//            filter reads the caller's dtype (through the flip) and writes float64; the last interpolation rounds into the caller's dtype.
//            For int16 / uint8 an axis with m == n is skipped: its exact result is the input sample.
//   prefilter a serial recurrence along a line, one lane per line.  With a stride between the line's samples (inner > 1) adjacent lanes hold
//            adjacent lines and every step of the recurrence is a coalesced row (rz_filter_strided_kernel).  Along the contiguous axis
//            (inner == 1) a wave takes 64 lines and moves them through LDS in 64 x 32 tiles: loads and stores are 256-byte runs, the lane
//            walks its own padded LDS row (rz_filter_rows_kernel).
//            The causal start sum stops after 64 terms: |z|^64 < 1e-36 of the line's magnitude.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "common.h"
#include "../../include/pointseg_prepare.h"

namespace ps {

namespace {

constexpr int kStartTerms = 64;  // terms of the causal start sum (all of them for lines up to 66 samples)
constexpr int kRowLines = 64;    // lines per workgroup (one wave) of the contiguous-axis filter
constexpr int kRowChunk = 32;    // samples per line and LDS tile

struct RzTap {
    double w[4];
    int idx[4];  // idx[0] < 0: the output index lies past the last sample by rounding -- its voxels are 0
};

struct RzDims {
    int n[3], m[3];
};

// the constants of the recurrence for one line length, formed on the host in double
struct RzPole {
    double z, iz, gain, zn1, z2n, zq;  // pole, 1 / z, (1 - z)(1 - 1 / z), z^(n-1), z^(2n-2), z / (z^2 - 1)
};

RzPole pole_for(int n)
{
    RzPole p;
    p.z = std::sqrt(3.0) - 2.0;
    p.iz = 1.0 / p.z;
    p.gain = (1.0 - p.z) * (1.0 - 1.0 / p.z);
    p.zn1 = std::pow(p.z, n - 1);
    p.z2n = std::pow(p.z, 2 * n - 2);
    p.zq = p.z / (p.z * p.z - 1.0);
    return p;
}

// ---- taps -------------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int rz_mirror(int i, int n)
{
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// grid (ceil(max m / 256), 3): axis blockIdx.y
__global__ __launch_bounds__(256) void rz_taps_kernel(RzTap* __restrict__ t0, RzTap* __restrict__ t1, RzTap* __restrict__ t2, RzDims d, int order)
{
    const int a = blockIdx.y;
    const int n = d.n[a], m = d.m[a];
    RzTap* tab = a == 0 ? t0 : a == 1 ? t1 : t2;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const double scale = m > 1 ? (double)(n - 1) / (double)(m - 1) : 0.0;
    const double cc = (double)j * scale;
    RzTap t;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t.w[k] = 0.0;
        t.idx[k] = 0;
    }
    if (cc > (double)(n - 1)) {
        t.idx[0] = -1;
    } else if (order == 0) {
        const int i = (int)floor(cc + 0.5);
        t.idx[0] = i < n ? i : n - 1;
        t.w[0] = 1.0;
    } else {
        const double f = floor(cc), x = cc - f, u = 1.0 - x;
        t.w[0] = u * u * u / 6.0;
        t.w[1] = (3.0 * x * x * x - 6.0 * x * x + 4.0) / 6.0;
        t.w[2] = (-3.0 * x * x * x + 3.0 * x * x + 3.0 * x + 1.0) / 6.0;
        t.w[3] = x * x * x / 6.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) t.idx[k] = rz_mirror((int)f - 1 + k, n);
    }
    tab[j] = t;
}

// ---- output conversion ------------------------------------------------------------------------------------------------------------------

template <class T>
__device__ __forceinline__ T rz_round(double v)
{
    if (std::is_same<T, float>::value) return (T)(float)v;
    const double lo = std::is_same<T, int16_t>::value ? -32768.0 : 0.0, hi = std::is_same<T, int16_t>::value ? 32767.0 : 255.0;
    double s = v > 0.0 ? v + 0.5 : v - 0.5;
    s = s < lo ? lo : s;
    s = s > hi ? hi : s;
    return (T)s;  // (the conversion truncates)
}

template <class T>
__device__ __forceinline__ T rz_clamp(T x, bool clamp, double lo, double hi)
{
    if (!clamp) return x;
    double v = (double)x;
    v = v < lo ? lo : v;
    v = v > hi ? hi : v;
    return (T)v;
}

// ---- order 0 ----------------------------------------------------------------------------------------------------------------------------

template <class T>
__global__ __launch_bounds__(256) void rz_gather_kernel(const T* __restrict__ in, T* __restrict__ out, const RzTap* __restrict__ t0,
                                                        const RzTap* __restrict__ t1, const RzTap* __restrict__ t2, RzDims d, unsigned flip,
                                                        unsigned total, bool clamp, double lo, double hi)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    const unsigned j2 = t % (unsigned)d.m[2], q = t / (unsigned)d.m[2], j1 = q % (unsigned)d.m[1], j0 = q / (unsigned)d.m[1];
    int i0 = t0[j0].idx[0], i1 = t1[j1].idx[0], i2 = t2[j2].idx[0];
    T v = (T)0;
    if (i0 >= 0 && i1 >= 0 && i2 >= 0) {
        if (flip & 1u) i0 = d.n[0] - 1 - i0;
        if (flip & 2u) i1 = d.n[1] - 1 - i1;
        if (flip & 4u) i2 = d.n[2] - 1 - i2;
        v = in[((size_t)i0 * d.n[1] + i1) * d.n[2] + i2];
    }
    out[t] = rz_clamp(v, clamp, lo, hi);
}

// ---- order 3: the input as float64 (only in front of a first filter along the contiguous axis, or a first axis too short to filter) -----

template <class T>
__global__ __launch_bounds__(256) void rz_convert_kernel(const T* __restrict__ in, double* __restrict__ out, RzDims d, unsigned flip, unsigned total)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    unsigned i2 = t % (unsigned)d.n[2], q = t / (unsigned)d.n[2], i1 = q % (unsigned)d.n[1], i0 = q / (unsigned)d.n[1];
    if (flip & 1u) i0 = d.n[0] - 1 - i0;
    if (flip & 2u) i1 = d.n[1] - 1 - i1;
    if (flip & 4u) i2 = d.n[2] - 1 - i2;
    out[t] = (double)in[((size_t)i0 * d.n[1] + i1) * d.n[2] + i2];
}

// ---- order 3: prefilter along an axis with a stride (inner > 1) ----------------------------------------------------------------------------

// The volume is [outer, n, inner]; lane = line (o, r), its samples `inner` apart.  S == double: in place in c.  Otherwise the samples come
// from the caller's volume src of dims d (this volume's shape, the line along `axis`), read through the flip, and c is written only.
template <class S>
__global__ __launch_bounds__(256) void rz_filter_strided_kernel(const S* src, double* c, unsigned lines, int n, unsigned inner, int axis, RzDims d,
                                                                unsigned flip, RzPole p)
{
    const unsigned l = blockIdx.x * 256u + threadIdx.x;
    if (l >= lines) return;
    const unsigned o = l / inner, r = l - o * inner;
    double* dst = c + ((size_t)o * n * inner + r);
    const S* s;
    long long step;
    if constexpr (std::is_same<S, double>::value) {
        s = dst;
        step = inner;
    } else {
        // the line's first sample in the caller's volume: coordinates with the line's own set to 0, each reversed where the flip asks
        long long i[3], st[3] = {(long long)d.n[1] * d.n[2], d.n[2], 1};
        if (axis == 0) {
            i[0] = 0, i[1] = r / (unsigned)d.n[2], i[2] = r % (unsigned)d.n[2];
        } else if (axis == 1) {
            i[0] = o, i[1] = 0, i[2] = r;
        } else {
            i[0] = o / (unsigned)d.n[1], i[1] = o % (unsigned)d.n[1], i[2] = 0;
        }
        long long off = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) off += (((flip >> a) & 1u) ? d.n[a] - 1 - i[a] : i[a]) * st[a];
        step = ((flip >> axis) & 1u) ? -st[axis] : st[axis];
        s = src + off;
    }
    auto X = [&](int i) { return p.gain * (double)s[(long long)i * step]; };
    // causal start over the mirrored line
    double acc = X(0) + p.zn1 * X(n - 1);
    {
        double zi = p.z, zr = p.z2n * p.iz;  // z^i and z^(2n-2-i)
        const int h = n - 2 < kStartTerms ? n - 2 : kStartTerms;
        for (int i = 1; i <= h; ++i) {
            acc += (zi + zr) * X(i);
            zi *= p.z;
            zr *= p.iz;
        }
    }
    double prev = acc / (1.0 - p.z2n), before = prev;
    dst[0] = prev;
    for (int i0 = 1; i0 < n; i0 += 8) {  // eight loads in flight per lane in front of the dependent chain
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u < n) x[u] = X(i0 + u);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + u < n) {
                const double cur = x[u] + p.z * prev;
                dst[(size_t)(i0 + u) * inner] = cur;
                before = prev;
                prev = cur;
            }
    }
    double nxt = p.zq * (p.z * before + prev);
    dst[(size_t)(n - 1) * inner] = nxt;
    for (int i0 = n - 2; i0 >= 0; i0 -= 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 - u >= 0) x[u] = dst[(size_t)(i0 - u) * inner];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 - u >= 0) {
                nxt = p.z * (nxt - x[u]);
                dst[(size_t)(i0 - u) * inner] = nxt;
            }
    }
}

// ---- order 3: prefilter along the contiguous axis (inner == 1), float64 in place ----------------------------------------------------------

// c is [lines, n].  One wave per 64 lines; a 64 x 32 tile of them passes through LDS per step, the lane walks row `lane`.
__global__ __launch_bounds__(kRowLines) void rz_filter_rows_kernel(double* c, unsigned lines, int n, RzPole p)
{
    __shared__ double tile[kRowLines][kRowChunk + 1];
    const unsigned lane = threadIdx.x, line0 = blockIdx.x * (unsigned)kRowLines;
    auto load = [&](int i0) {
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kRowChunk; ++k) {
            const unsigned e = k * kRowLines + lane, ll = e / kRowChunk, col = e % kRowChunk;
            const unsigned L = line0 + ll;
            const int i = i0 + (int)col;
            tile[ll][col] = (L < lines && i < n) ? c[(size_t)L * n + i] : 0.0;
        }
        __syncthreads();
    };
    auto store = [&](int i0) {
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < kRowChunk; ++k) {
            const unsigned e = k * kRowLines + lane, ll = e / kRowChunk, col = e % kRowChunk;
            const unsigned L = line0 + ll;
            const int i = i0 + (int)col;
            if (L < lines && i < n) c[(size_t)L * n + i] = tile[ll][col];
        }
    };
    double* row = tile[lane];
    const unsigned mine = line0 + lane < lines ? line0 + lane : lines - 1;  // (a lane past the last line repeats it and stores nothing)
    // causal start over the mirrored line
    const int h = n - 2 < kStartTerms ? n - 2 : kStartTerms;
    double acc = p.zn1 * (p.gain * c[(size_t)mine * n + (n - 1)]);
    {
        double zi = p.z, zr = p.z2n * p.iz;
        for (int i0 = 0; i0 <= h; i0 += kRowChunk) {
            load(i0);
            for (int col = 0; col < kRowChunk; ++col) {
                const int i = i0 + col;
                if (i == 0) {
                    acc += p.gain * row[col];
                } else if (i <= h) {
                    acc += (zi + zr) * (p.gain * row[col]);
                    zi *= p.z;
                    zr *= p.iz;
                }
            }
        }
    }
    double prev = acc / (1.0 - p.z2n), before = prev;
    for (int i0 = 0; i0 < n; i0 += kRowChunk) {
        load(i0);
        for (int col = 0; col < kRowChunk; ++col) {
            const int i = i0 + col;
            if (i == 0) {
                row[col] = prev;
            } else if (i < n) {
                const double cur = p.gain * row[col] + p.z * prev;
                row[col] = cur;
                before = prev;
                prev = cur;
            }
        }
        store(i0);
    }
    double nxt = p.zq * (p.z * before + prev);
    for (int i0 = (n - 1) / kRowChunk * kRowChunk; i0 >= 0; i0 -= kRowChunk) {
        load(i0);
        for (int col = kRowChunk - 1; col >= 0; --col) {
            const int i = i0 + col;
            if (i == n - 1) {
                row[col] = nxt;
            } else if (i < n - 1) {
                nxt = p.z * (nxt - row[col]);
                row[col] = nxt;
            }
        }
        store(i0);
    }
}

// ---- order 3: the four taps along one axis ---------------------------------------------------------------------------------------------------

// src [outer, n, inner] -> dst [outer, m, inner]; O == double: the next axis' coefficients, otherwise the caller's volume (rounded, clipped)
template <class O>
__global__ __launch_bounds__(256) void rz_interp_kernel(const double* __restrict__ src, O* __restrict__ dst, const RzTap* __restrict__ tap, unsigned n,
                                                        unsigned m, unsigned inner, unsigned total, bool clamp, double lo, double hi)
{
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    const unsigned r = t % inner, q = t / inner, j = q % m, o = q / m;
    const RzTap tp = tap[j];
    double v = 0.0;
    if (tp.idx[0] >= 0) {
        const double* s = src + ((size_t)o * n * inner + r);
        v = tp.w[0] * s[(size_t)tp.idx[0] * inner] + tp.w[1] * s[(size_t)tp.idx[1] * inner] + tp.w[2] * s[(size_t)tp.idx[2] * inner] +
            tp.w[3] * s[(size_t)tp.idx[3] * inner];
    }
    if constexpr (std::is_same<O, double>::value) dst[t] = v;
    else dst[t] = rz_clamp(rz_round<O>(v), clamp, lo, hi);
}

size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }

unsigned blocks256(size_t n) { return (unsigned)((n + 255) / 256); }

// the order-3 chain for one dtype; A / B: the two float64 scratch volumes
template <class T>
void zoom_cubic(hipStream_t sm, const T* in, T* out, const RzDims& d, const int* seq, int n_seq, const RzTap* const* taps, unsigned flip, bool clamp,
               double lo, double hi, double* A, double* B, int& launches)
{
    int cur[3] = {d.n[0], d.n[1], d.n[2]};
    double *here = A, *other = B;
    for (int k = 0; k < n_seq; ++k) {
        const int a = seq[k], n = cur[a];
        const size_t outer = a == 0 ? 1 : a == 1 ? (size_t)cur[0] : (size_t)cur[0] * cur[1];
        const size_t inner = a == 0 ? (size_t)cur[1] * cur[2] : a == 1 ? (size_t)cur[2] : 1;
        const size_t lines = outer * inner, vol = lines * n;
        const RzPole p = pole_for(n);
        const bool fused = k == 0 && n >= 2 && inner > 1;  // the first filter reads the caller's volume itself
        if (k == 0 && !fused) {
            hipLaunchKernelGGL(rz_convert_kernel<T>, dim3(blocks256(vol)), dim3(256), 0, sm, in, here, d, flip, (unsigned)vol);
            ++launches;
        }
        if (n >= 2) {
            if (fused)
                hipLaunchKernelGGL(rz_filter_strided_kernel<T>, dim3(blocks256(lines)), dim3(256), 0, sm, in, here, (unsigned)lines, n, (unsigned)inner, a, d,
                                   flip, p);
            else if (inner > 1)
                hipLaunchKernelGGL(rz_filter_strided_kernel<double>, dim3(blocks256(lines)), dim3(256), 0, sm, static_cast<const double*>(nullptr), here,
                                   (unsigned)lines, n, (unsigned)inner, a, d, 0u, p);
            else
                hipLaunchKernelGGL(rz_filter_rows_kernel, dim3((unsigned)((lines + kRowLines - 1) / kRowLines)), dim3(kRowLines), 0, sm, here, (unsigned)lines,
                                   n, p);
            ++launches;
        }
        const int m = d.m[a];
        const size_t total = outer * m * inner;
        if (k == n_seq - 1)
            hipLaunchKernelGGL(rz_interp_kernel<T>, dim3(blocks256(total)), dim3(256), 0, sm, here, out, taps[a], (unsigned)n, (unsigned)m, (unsigned)inner,
                               (unsigned)total, clamp, lo, hi);
        else
            hipLaunchKernelGGL(rz_interp_kernel<double>, dim3(blocks256(total)), dim3(256), 0, sm, here, other, taps[a], (unsigned)n, (unsigned)m,
                               (unsigned)inner, (unsigned)total, false, 0.0, 0.0);
        ++launches;
        cur[a] = m;
        std::swap(here, other);
    }
}

template <class T>
void zoom_gather(hipStream_t sm, const T* in, T* out, const RzDims& d, const RzTap* const* taps, unsigned flip, bool clamp, double lo, double hi)
{
    const size_t total = (size_t)d.m[0] * d.m[1] * d.m[2];
    hipLaunchKernelGGL(rz_gather_kernel<T>, dim3(blocks256(total)), dim3(256), 0, sm, in, out, taps[0], taps[1], taps[2], d, flip, (unsigned)total, clamp, lo,
                       hi);
}

}  // namespace

}  // namespace ps

extern "C" int ps_volume_zoom(ps_context* c, const void* in, int32_t dtype, int64_t n0, int64_t n1, int64_t n2, int32_t order, int64_t m0, int64_t m1,
                              int64_t m2, uint32_t flip_axes, int32_t clamp, double clamp_lo, double clamp_hi, void* out, void* scratch,
                              int64_t* scratch_bytes)
{
    using namespace ps;
    // every argument error is found here, before anything is enqueued
    PS_CHECK(c && scratch_bytes, "ps_volume_zoom: NULL argument");
    PS_CHECK(!scratch || (in && out), "ps_volume_zoom: NULL volume (in and out may be NULL only in the call that sizes the scratch)");
    PS_CHECK(dtype == PS_VOLUME_I16 || dtype == PS_VOLUME_F32 || dtype == PS_VOLUME_U8,
             "ps_volume_zoom: dtype = %d is none of PS_VOLUME_I16, PS_VOLUME_F32, PS_VOLUME_U8", (int)dtype);
    PS_CHECK(order == 0 || order == 3, "ps_volume_zoom: order = %d, must be 0 or 3", (int)order);
    const int64_t lim = 1ll << 31, dim = 1ll << 30;  // a dimension <= 2^30: the mirror period 2 n - 2 stays an int
    PS_CHECK(n0 >= 1 && n1 >= 1 && n2 >= 1 && n0 <= dim && n1 <= dim && n2 <= dim && n0 * n1 < lim && n0 * n1 * n2 < lim,
             "ps_volume_zoom: input %lld x %lld x %lld (every dimension in [1, 2^30], n0 * n1 * n2 < 2^31)", (long long)n0, (long long)n1, (long long)n2);
    PS_CHECK(m0 >= 1 && m1 >= 1 && m2 >= 1 && m0 <= dim && m1 <= dim && m2 <= dim && m0 * m1 < lim && m0 * m1 * m2 < lim,
             "ps_volume_zoom: output %lld x %lld x %lld (every dimension in [1, 2^30], m0 * m1 * m2 < 2^31)", (long long)m0, (long long)m1, (long long)m2);
    PS_CHECK(flip_axes < 8u, "ps_volume_zoom: flip_axes = %u has bits above the three axes", (unsigned)flip_axes);
    if (clamp) {
        PS_CHECK(clamp_lo <= clamp_hi, "ps_volume_zoom: clamp [%g, %g] is empty or NaN", clamp_lo, clamp_hi);
        if (dtype != PS_VOLUME_F32) {
            const double tlo = dtype == PS_VOLUME_I16 ? -32768.0 : 0.0, thi = dtype == PS_VOLUME_I16 ? 32767.0 : 255.0;
            PS_CHECK(clamp_lo >= tlo && clamp_hi <= thi && clamp_lo == std::floor(clamp_lo) && clamp_hi == std::floor(clamp_hi),
                     "ps_volume_zoom: clamp [%g, %g] must be integers inside the dtype's range [%g, %g]", clamp_lo, clamp_hi, tlo, thi);
        }
    }
    RzDims d = {{(int)n0, (int)n1, (int)n2}, {(int)m0, (int)m1, (int)m2}};
    // the order-3 sequence of axes: the ones that shrink first, so that no intermediate volume is larger than the input or the output;
    // integer dtypes skip an axis that keeps its length
    int seq[3], n_seq = 0;
    if (order == 3) {
        for (int a = 0; a < 3; ++a)
            if (d.m[a] < d.n[a]) seq[n_seq++] = a;
        for (int a = 0; a < 3; ++a)
            if (d.m[a] > d.n[a] || (d.m[a] == d.n[a] && dtype == PS_VOLUME_F32)) seq[n_seq++] = a;
    }
    size_t need[2] = {0, 0};  // elements of the two float64 volumes: the stages alternate between them
    {
        size_t cur[3] = {(size_t)n0, (size_t)n1, (size_t)n2};
        for (int k = 0; k < n_seq; ++k) {
            need[k & 1] = std::max(need[k & 1], cur[0] * cur[1] * cur[2]);
            cur[seq[k]] = (size_t)d.m[seq[k]];
        }
    }
    // the scratch: taps of the three axes | float64 volume A | float64 volume B
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += pad256(bytes); return o; };
    const size_t o_t0 = take(sizeof(RzTap) * (size_t)m0), o_t1 = take(sizeof(RzTap) * (size_t)m1), o_t2 = take(sizeof(RzTap) * (size_t)m2);
    const size_t o_a = take(sizeof(double) * need[0]), o_b = take(sizeof(double) * need[1]);
    if (!scratch) {  // the first call of the two-call protocol
        *scratch_bytes = (int64_t)off;
        return PS_OK;
    }
    PS_CHECK(*scratch_bytes >= (int64_t)off, "ps_volume_zoom: *scratch_bytes = %lld, this call needs %lld", (long long)*scratch_bytes, (long long)off);
    PS_CHECK((reinterpret_cast<uintptr_t>(scratch) & 255) == 0, "ps_volume_zoom: scratch must be 256-byte aligned");
    char* base = static_cast<char*>(scratch);
    RzTap* tabs[3] = {reinterpret_cast<RzTap*>(base + o_t0), reinterpret_cast<RzTap*>(base + o_t1), reinterpret_cast<RzTap*>(base + o_t2)};
    double *A = reinterpret_cast<double*>(base + o_a), *B = reinterpret_cast<double*>(base + o_b);
    const bool cl = clamp != 0;

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    {
        Stage stg(c, "volume_zoom", 1);
        int launches = 1;
        const int64_t mmax = std::max(m0, std::max(m1, m2));
        hipLaunchKernelGGL(rz_taps_kernel, dim3(blocks256((size_t)mmax), 3), dim3(256), 0, sm, tabs[0], tabs[1], tabs[2], d, n_seq ? 3 : 0);
        if (n_seq == 0) {
            if (dtype == PS_VOLUME_I16) zoom_gather(sm, static_cast<const int16_t*>(in), static_cast<int16_t*>(out), d, tabs, flip_axes, cl, clamp_lo, clamp_hi);
            else if (dtype == PS_VOLUME_U8) zoom_gather(sm, static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), d, tabs, flip_axes, cl, clamp_lo, clamp_hi);
            else zoom_gather(sm, static_cast<const float*>(in), static_cast<float*>(out), d, tabs, flip_axes, cl, clamp_lo, clamp_hi);
            ++launches;
        } else if (dtype == PS_VOLUME_I16) {
            zoom_cubic(sm, static_cast<const int16_t*>(in), static_cast<int16_t*>(out), d, seq, n_seq, tabs, flip_axes, cl, clamp_lo, clamp_hi, A, B, launches);
        } else if (dtype == PS_VOLUME_U8) {
            zoom_cubic(sm, static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), d, seq, n_seq, tabs, flip_axes, cl, clamp_lo, clamp_hi, A, B, launches);
        } else {
            zoom_cubic(sm, static_cast<const float*>(in), static_cast<float*>(out), d, seq, n_seq, tabs, flip_axes, cl, clamp_lo, clamp_hi, A, B, launches);
        }
        PS_HIP(hipGetLastError());
        stg.n = launches;
    }
    return PS_OK;
}
