// conv3d_train_bf16.hip -- the convolution's weight and bias gradient on v_mfma_f32_32x32x16_bf16: the PS_PREC_BF16X3 and PS_PREC_BF16 modes
// of ps_conv3d_bwd_weight_prec (include/pointseg_saliency_train_precision.h).  The data gradient of those modes is
// conv3d_bf16.hip's kernel with its gather policy.
//
// The geometry is conv3d_train.hip's conv3d_bwd_weight_kernel: dw[(t, ci), co] = sum over voxels of in[v, (t, ci)] . dy[v, co], rows (t, ci)
// plus the row of ones (the bias gradient), a workgroup sums one slab of 4096 output voxels of one sample in chunks of 32 voxels -- a fresh
// accumulator per chunk, added to the running one -- with the voxels' input corners double-buffered in LDS, and writes its [rows, columns]
// tile to scratch; reduce_partials.h adds the slabs.  What differs is conv3d_bf16.hip's: an operand element is split (P = 3) or rounded
// (P = 1) once between the fetch registers and LDS, and both tiles are k-contiguous planes of bfloat16 with the 80-byte pitch, A as
// [row][32 voxels] and dy as [column][32 voxels], so a lane's MFMA fragment is one 16-byte read per plane.
// k is a voxel here and memory is channel-contiguous per voxel, so the transposition happens in the fetch: thread (lane = row, wave) fetches
// its row's value of the 8 CONSECUTIVE voxels 8 * wave .. 8 * wave + 7 of the chunk -- adjacent lanes adjacent channels of one voxel, as in the
// fp32 kernel -- which is exactly one b3_split8 and one 16-byte LDS store per plane.  A wave owns 32 rows and all NT column tiles.
#include "conv3d_kit.h"

namespace ps {

namespace {

template <int P, int RT, int NT>
__global__ __launch_bounds__(256) void conv3d_bwd_weight_b_kernel(BwdWeightArgs a)
{
    constexpr int M = 64 * RT, N = 32 * NT;
    constexpr int BK = kBKC * N / 256;  // consecutive voxels of one column per thread: 4 or 8
    __shared__ __attribute__((aligned(16))) unsigned As[P][M * kPW];
    __shared__ __attribute__((aligned(16))) unsigned Bs[P][N * kPW];
    __shared__ int4 vox[2][kBKC];  // the input corner of the voxel's receptive field (z, y, x) and whether the voxel exists

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int mt = blockIdx.x % a.mtiles, pidx = blockIdx.x / a.mtiles;
    const int b = pidx / a.slabs, slab = pidx - b * a.slabs;
    const int m0 = mt * M, n0 = blockIdx.y * N;
    const int Vo = a.Do * a.Ho * a.Wo;
    const int v0 = slab * kWSlab, v1 = min(Vo, v0 + kWSlab);
    const int nchunks = (v1 - v0 + kBKC - 1) / kBKC;
    const int cin = a.C1 + a.C2;
    const size_t xs = (size_t)a.Ds * a.Hs * a.Ws;
    const float* dyb = a.dy + (size_t)b * Vo * a.cout;

    // this thread's rows: kind 0 = none, 1 = a kernel row, 2 = the row of ones
    int kind[RT], rdz[RT], rdy[RT], rdx[RT], rld[RT];
    const float* rsrc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int lr = m0 + rt * 64 + lane, row = a.r0 + lr;
        kind[rt] = lr >= a.nrows ? 0 : (row < a.Ktot ? 1 : 2);
        const int tap = kind[rt] == 1 ? row / cin : 0, ci = kind[rt] == 1 ? row - tap * cin : 0;
        rdx[rt] = (tap % a.kw) * a.dil, rdy[rt] = (tap / a.kw % a.kh) * a.dil, rdz[rt] = (tap / (a.kw * a.kh)) * a.dil;
        const bool second = ci >= a.C1;
        rsrc[rt] = second ? a.x2 + (size_t)b * xs * a.C2 + (ci - a.C1) : a.x + (size_t)b * xs * a.C1 + ci;
        rld[rt] = second ? a.C2 : a.C1;
    }
    const int bcol = t % N, bk0 = (t / N) * BK;
    const bool bin = n0 + bcol < a.cout;
    const unsigned upm = div_magic(a.up);  // (used where up > 1)

    auto put_vox = [&](int chunk) {
        if (t < kBKC) {
            const int v = v0 + chunk * kBKC + t;
            int4 vi = {0, 0, 0, 0};
            if (v < v1) vi = {v / (a.Wo * a.Ho) * a.stride - a.pd, v / a.Wo % a.Ho * a.stride - a.ph, v % a.Wo * a.stride - a.pw, 1};
            vox[chunk & 1][t] = vi;
        }
    };

    float areg[RT][8], breg[BK];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int4 vi = vox[chunk & 1][8 * wave + i];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                int z = vi.x + rdz[rt], y = vi.y + rdy[rt], x = vi.z + rdx[rt];
                const bool ok = kind[rt] == 1 && vi.w && (unsigned)z < (unsigned)a.D && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
                if (!ok) z = y = x = 0;
                if (a.up > 1) z = div_by(z, a.up, upm), y = div_by(y, a.up, upm), x = div_by(x, a.up, upm);
                const float one = (kind[rt] == 2 && vi.w) ? 1.f : 0.f;
                // (the load is unconditional: without `ok` it reads voxel 0 of the row's source, which exists, and is dropped)
                const float v = rsrc[rt][(size_t)((z * a.Hs + y) * a.Ws + x) * rld[rt]];
                areg[rt][i] = ok ? v : one;
            }
        }
        const int vb = v0 + chunk * kBKC + bk0;
#pragma unroll
        for (int i = 0; i < BK; ++i) breg[i] = (bin && vb + i < v1) ? dyb[(size_t)(vb + i) * a.cout + n0 + bcol] : 0.f;
    };
    // split or round the fetched chunk into the planes
    auto stage = [&]() {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const BPlanes<P> p = b3_split8<P>(areg[rt]);
#pragma unroll
            for (int pl = 0; pl < P; ++pl) *reinterpret_cast<uint4*>(&As[pl][(rt * 64 + lane) * kPW + wave * 4]) = p.p[pl];
        }
        stage_b<P, BK>(breg, &Bs[0][bcol * kPW + bk0 / 2], N * kPW);
    };

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int c32 = lane & 31, hl = lane >> 5;
    const bool mma = wave * 32 < M;  // (wave uniform: the 64-row form keeps two of its four waves for the fetch alone)
    const int fa = (wave * 32 + c32) * kPW + hl * 4, fb = c32 * kPW + hl * 4;
    put_vox(0);
    __syncthreads();
    fetch(0);
#pragma unroll 1
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        stage();
        if (chunk + 1 < nchunks) put_vox(chunk + 1);
        __syncthreads();
        if (chunk + 1 < nchunks) fetch(chunk + 1);
        if (mma) {
            f32x16 part[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) part[j][r] = 0.f;
#pragma unroll
            for (int s = 0; s < kBKC / 16; ++s) {
                BPlanes<P> af;
#pragma unroll
                for (int pl = 0; pl < P; ++pl) af.p[pl] = *reinterpret_cast<const uint4*>(&As[pl][fa + s * 8]);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    BPlanes<P> bf;
#pragma unroll
                    for (int pl = 0; pl < P; ++pl) bf.p[pl] = *reinterpret_cast<const uint4*>(&Bs[pl][fb + j * 32 * kPW + s * 8]);
                    part[j] = b3_mfma6<P>(af, bf, part[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] += part[j];
        }
        __syncthreads();
    }
    if (!mma) return;

    float* pb = a.part + (size_t)pidx * a.nrows * a.cout;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = n0 + j * 32 + c32;
        if (col >= a.cout) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lr = c_row_b(m0 + wave * 32, r, hl);
            if (lr < a.nrows) pb[(size_t)lr * a.cout + col] = acc[j][r];
        }
    }
}

template <int P, int RT, int NT>
void launch(hipStream_t sm, BwdWeightArgs& a)
{
    a.mtiles = ceil_div(a.nrows, 64 * RT);
    const dim3 grid((unsigned)((int64_t)a.mtiles * a.B * a.slabs), (unsigned)ceil_div(a.cout, 32 * NT));
    hipLaunchKernelGGL((conv3d_bwd_weight_b_kernel<P, RT, NT>), grid, dim3(256), 0, sm, a);
}

// (conv3d_kit.h's form rule; P = 3 comes with more than 64 rows, or with the bias row alone, and has the 128-row forms only:
// conv3d_bwd_weight_split_pays)
template <int P>
void launch_p(hipStream_t sm, BwdWeightArgs& a)
{
    conv_form_b<P == 1>(a.nrows > 64, a.cout, [&](auto rt, auto nt) { launch<P, decltype(rt)::value, decltype(nt)::value>(sm, a); });
}

}  // namespace

void conv3d_bwd_weight_b_launch(hipStream_t sm, BwdWeightArgs& a, int precision)
{
    if (precision == PS_PREC_BF16) launch_p<1>(sm, a);
    else launch_p<3>(sm, a);
}

}  // namespace ps
