// attpool_lane.hip -- level-0 attentive pooling (d = 16, K = 16, direct full-Wfc formulation) on the vector ALU, one lane per
// (point, neighbour) row.
//
// The same arithmetic as att_direct_kernel<16, STAGE, 16, ..> (attpool.hip), in the same order, without the matrix pipe: at d = 16 / h = 8
// half the columns of every LocSE / mlp2 MFMA tile are padding, every 16-lane group of a wave recomputes the neighbour geometry, and half of
// the vector instructions only stage fragments.  Here lane l of a wave owns neighbour k = l & 15 of point t + (l >> 4) -- four points per
// wave iteration -- and runs its row's three products as k-ordered fma chains (bit for bit what v_mfma_f32_16x16x4_f32 computes) with the
// weights as SCALAR operands: the 416 floats of a stage (kLaneImageFloats, packed by pack_lane_image) are read with scalar loads, 32 floats
// at a time, inside the iteration -- hoisted out of the loop they do not fit the scalar register file.  Softmax and weighted sum run
// transposed: scores, then values, go through one per-wave LDS tile, lane (point, channel) reads its 16 rows and reduces them in registers
// in att_direct_kernel's summation order (four in-order partial sums of four rows, then (0 + 1) + (2 + 3)).
#include "attpool.h"
#include "mfma_tile.h"

namespace ps {

void pack_lane_image(const float* W1, const float* b1, const float* W2, const float* b2, const float* wfc_scaled, float* out)
{
    std::memcpy(out + kLaneB1, b1, sizeof(float) * 8);
    std::memcpy(out + kLaneW1, W1, sizeof(float) * 80);
    if (b2) std::memcpy(out + kLaneB2, b2, sizeof(float) * 8);
    else std::memset(out + kLaneB2, 0, sizeof(float) * 8);
    if (W2) std::memcpy(out + kLaneW2, W2, sizeof(float) * 64);
    else std::memset(out + kLaneW2, 0, sizeof(float) * 64);
    std::memcpy(out + kLaneWfc, wfc_scaled, sizeof(float) * 256);
}

namespace {

struct AttLaneArgs {
    const float* xyz;
    const int32_t* idx;
    const int32_t* order;
    const float* f;
    const float* w;  // the stage's image (pack_lane_image)
    float* agg;
    int n_total, n_cloud, ldf;
};

constexpr int kLaneWaves = 4;          // waves per workgroup
constexpr int kLanePts = 4;            // points per wave iteration
constexpr int kLaneMaxBlocks = 256 * 8;
constexpr int kLanePitch = 17;         // floats per row of the [64 x 16] transpose tile: odd, so rows and columns are both conflict free

// (the chunk numbers of the kernel: chunk c is floats [32c, 32c + 32) of the image)
static_assert(kLaneB1 == 0 && kLaneW1 == 8 && kLaneB2 == 88 && kLaneW2 == 96 && kLaneWfc == 160 && kLaneImageFloats == 13 * 32, "att_lane_kernel: image layout");

using cfloat = const float __attribute__((address_space(4)));  // constant address space: a uniform load from it is a scalar load
using cfloat2 = const f32x2 __attribute__((address_space(4)));

__device__ __forceinline__ f32x2 fma2(float x, f32x2 w, f32x2 acc) { return __builtin_elementwise_fma(f32x2{x, x}, w, acc); }
__device__ __forceinline__ f32x2 leaky2(f32x2 v) { return f32x2{leaky02(v.x), leaky02(v.y)}; }

template <int STAGE>
__global__ __launch_bounds__(kLaneWaves * 64) void att_lane_kernel(AttLaneArgs a)
{
    __shared__ float smem[kLaneWaves * 64 * kLanePitch];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int pi = lane >> 4, k = lane & 15;  // phase 1: neighbour k of point pi; phase 2: channel k of point pi
    float* T = smem + wave * (64 * kLanePitch);
    float* t_row = T + lane * kLanePitch;             // this lane's row
    const float* t_col = T + (pi * 16) * kLanePitch + k;  // column k of this lane's point
    cfloat* wimg = (cfloat*)(uintptr_t)a.w;

    const bool one_cloud = a.n_total == a.n_cloud;
    // four consecutive points (of a contiguous eighth of the leaf order per XCD, as PointWalk) per wave iteration
    const int per_xcd = ((((a.n_total + 7) >> 3) + kLanePts - 1) / kLanePts) * kLanePts;
    const int w_end = min(a.n_total, (int)((blockIdx.x & 7) + 1) * per_xcd), w_slots = gridDim.x >> 3;
    for (int t = (int)(blockIdx.x & 7) * per_xcd + ((int)(blockIdx.x >> 3) * kLaneWaves + wave) * kLanePts; t < w_end; t += w_slots * kLaneWaves * kLanePts) {
        const int ti = min(t + pi, w_end - 1);  // (a point past the end: recomputes the last one, stores nothing)
        unsigned p, base;
        if (one_cloud) {
            p = a.order ? (unsigned)a.order[ti] : (unsigned)ti;
            base = 0u;
        } else {
            base = ((unsigned)ti / (unsigned)a.n_cloud) * (unsigned)a.n_cloud;
            p = a.order ? base + (unsigned)a.order[ti] : (unsigned)ti;
        }
        const float* cp = a.xyz + 3u * p;
        const float cx = cp[0], cy = cp[1], cz = cp[2];
        const unsigned nb = base + (unsigned)a.idx[p * 16u + (unsigned)k];
        const float* np = a.xyz + 3u * nb;
        const float nx = np[0], ny = np[1], nz = np[2];
        const float4* fr = reinterpret_cast<const float4*>(a.f + nb * (unsigned)a.ldf);
        const float4 fa = fr[0], fb = fr[1];
        const float rx = cx - nx, ry = cy - ny, rz = cz - nz;
        const float dis = __builtin_amdgcn_sqrtf(rx * rx + ry * ry + rz * rz);
        const float enc[10] = {dis, rx, ry, rz, cx, cy, cz, nx, ny, nz};

        // Weights: 13 chunks of 32 floats (two s_load_dwordx16 each), two chunks live in scalar registers -- the next one is fetched while this one feeds
        // its 16 packed fmas.  `fetch` ties the loads to a value of the chunk before, so they stay inside the iteration and in this order.
        f32x2 w[2][16];
        auto fetch = [&](int c, f32x2 (&dst)[16], auto& after) {
            cfloat* wp = wimg;
            asm volatile("" : "+s"(wp), "+v"(after));
            cfloat2* w2 = reinterpret_cast<cfloat2*>(wp) + c * 16;
#pragma unroll
            for (int j = 0; j < 16; ++j) dst[j] = w2[j];
        };
        auto mac4 = [](float xv, const f32x2* wr, f32x2 (&acc)[4]) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fma2(xv, wr[j], acc[j]);
        };
        // ---- LFA mlp1: f_xyz = lrelu(b1 + enc . W1), the bias seeds the chain.  Chunks 0-2: b1 | W1 rows 0-2, rows 3-6, rows 7-9 | b2 ----
        int tie = ti;
        fetch(0, w[0], tie);
        fetch(1, w[1], tie);
        f32x2 fx[4], g2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) fx[j] = w[0][j];
#pragma unroll
        for (int q = 0; q < 3; ++q) mac4(enc[q], &w[0][4 + 4 * q], fx);
        fetch(2, w[0], fx[0]);
#pragma unroll
        for (int q = 3; q < 7; ++q) mac4(enc[q], &w[1][4 * (q - 3)], fx);
        fetch(STAGE == 2 ? 3 : 5, w[1], fx[0]);
#pragma unroll
        for (int q = 7; q < 10; ++q) mac4(enc[q], &w[0][4 * (q - 7)], fx);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g2[j] = w[0][12 + j];
            fx[j] = leaky2(fx[j]);
        }
        if constexpr (STAGE == 2) {  // ---- LFA mlp2: lrelu(b2 + f_xyz . W2).  Chunks 3-4: W2 rows 0-3, rows 4-7 ----
            fetch(4, w[0], g2[0]);
#pragma unroll
            for (int q = 0; q < 4; ++q) mac4(q & 1 ? fx[q >> 1].y : fx[q >> 1].x, &w[1][4 * q], g2);
            fetch(5, w[1], g2[0]);
#pragma unroll
            for (int q = 4; q < 8; ++q) mac4(q & 1 ? fx[q >> 1].y : fx[q >> 1].x, &w[0][4 * (q - 4)], g2);
#pragma unroll
            for (int j = 0; j < 4; ++j) fx[j] = leaky2(g2[j]);
        }
        // ---- scores s = [f_nb | f_xyz] . Wfc' (Wfc times log2 e), seeded with 0.  Chunks 5-12: two rows of Wfc' each, chunk 5 is in w[1] ----
        const float x[16] = {fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w, fx[0].x, fx[0].y, fx[1].x, fx[1].y, fx[2].x, fx[2].y, fx[3].x, fx[3].y};
        f32x2 s[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] = f32x2{0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < 7) fetch(6 + i, w[i & 1], s[0]);
            const f32x2* wr = w[(i + 1) & 1];
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = fma2(x[2 * i], wr[j], s[j]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = fma2(x[2 * i + 1], wr[8 + j], s[j]);
        }
        // ---- transpose through the wave's tile: lane (point, channel) takes the 16 scores, then the 16 values, of its column ----
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            t_row[2 * j] = s[j].x;
            t_row[2 * j + 1] = s[j].y;
        }
        wave_lds_sync();
        float sc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = t_col[r * kLanePitch];
        wave_lds_sync();
#pragma unroll
        for (int q = 0; q < 16; ++q) t_row[q] = x[q];
        wave_lds_sync();
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = t_col[r * kLanePitch];
        wave_lds_sync();  // the tile is overwritten by the next iteration
        // softmax over the 16 rows and weighted sum, in att_direct_kernel's order: rows 4g .. 4g+3 in order, then (0 + 1) + (2 + 3)
        float m = sc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) m = fmaxf(m, sc[r]);
        float ss[4], num[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            ss[g] = 0.f;
            num[g] = 0.f;
#pragma unroll
            for (int r = 4 * g; r < 4 * g + 4; ++r) {
                const float e = __builtin_amdgcn_exp2f(sc[r] - m);
                ss[g] += e;
                num[g] = __builtin_fmaf(e, v[r], num[g]);
            }
        }
        const float ssum = (ss[0] + ss[1]) + (ss[2] + ss[3]);
        const float nsum = (num[0] + num[1]) + (num[2] + num[3]);
        if (t + pi < w_end) a.agg[p * 16u + (unsigned)k] = nsum * __builtin_amdgcn_rcpf(ssum);
    }
}

}  // namespace

int att_lane_pass_points() { return kLaneMaxBlocks * kLaneWaves * kLanePts; }

bool att_lane_fits(const ps_context* c, const AttStage& s)
{
    return c->att_lane && s.wfull && s.lane && s.d == 16 && s.k == 16 && s.ldf >= 8 && s.ldf % 4 == 0 &&
           (uint64_t)s.n_total * (uint64_t)std::max(s.d, std::max(s.ldf, 3)) < (1ull << 32);
}

int att_lane_stage(ps_context* c, const AttStage& s)
{
    if (!(s.wfull && s.lane && s.d == 16 && s.k == 16)) {
        set_error("att_pool(lane): d_out %d, k_n %d -- the lane kernel is compiled for d_out 16, k_n 16 and the direct formulation only", s.d, s.k);
        return PS_EINVAL;
    }
    PS_CHECK((uint64_t)s.n_total * (uint64_t)std::max(s.d, std::max(s.ldf, 3)) < (1ull << 32), "att_pool(lane): level too large for 32-bit element offsets");
    PS_CHECK(s.ldf % 4 == 0 && s.ldf >= 8, "att_pool(lane): feature rows need a stride of whole float4s");
    if (s.n_total <= 0) return PS_OK;
    AttLaneArgs a;
    a.xyz = s.xyz; a.idx = s.idx; a.order = s.order; a.f = s.fg; a.w = s.lane; a.agg = s.agg;
    a.n_total = (int)s.n_total; a.n_cloud = (int)s.n_cloud; a.ldf = s.ldf;
    const int blocks = (std::min(ceil_div(a.n_total, kLaneWaves * kLanePts), kLaneMaxBlocks) + 7) & ~7;  // a multiple of 8 (one eighth of the points per XCD)
    if (s.lfa2) hipLaunchKernelGGL(att_lane_kernel<2>, dim3(blocks), dim3(kLaneWaves * 64), 0, c->stream, a);
    else hipLaunchKernelGGL(att_lane_kernel<1>, dim3(blocks), dim3(kLaneWaves * 64), 0, c->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

}  // namespace ps
