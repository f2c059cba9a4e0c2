// conv3d_bf16.hip -- conv3d.hip's implicit-GEMM 3-D convolution on v_mfma_f32_32x32x16_bf16 (b3_ops.h's fragment maps and split helpers):
// the PS_PREC_BF16X3 and PS_PREC_BF16 modes of ps_conv3d_prec and ps_saliency_forward_prec (include/pointseg_saliency_precision.h,
// DESIGN.md 4.15), and -- the same kernel with its gather policy GRAD -- the data gradient of ps_conv3d_bwd_data_prec in those modes
// (include/pointseg_saliency_train_precision.h).
//
// The frame is conv3d.hip's: Y[v, co] = sum over k of A[v, k] . Wm[k, co], k = tap * C_in + ci, TensorFlow's kernel buffer as the row-major
// [K, C_out] matrix, A never materialised; a workgroup of four waves owns 64 * RT output voxels and 32 * NT output channels, the rows' input
// corners live in LDS, K is walked in chunks of 32, the fetch of the next chunk is in flight during the chunk's MFMAs, and a chunk is summed
// in a fresh accumulator that is then added to the running one (the same bounded rounding chain).  What differs:
//   * An operand element is split (P = 3: b3_split_pair's exact truncating three-way split, the six piece products of b3_mfma6) or rounded
//     (P = 1: b3_rne_pair, round to nearest even) ONCE, between the fetch registers and LDS, and lies there as P planes of bfloat16.
//   * Both tiles are k-contiguous: A as [row][32 k], Wm transposed to [column][32 k], so a lane's MFMA fragment (8 consecutive k of its row
//     or column) is one 16-byte LDS read per plane.  The pitch is 80 bytes (kPW words): a ds_read_b128 is served in groups of 16 lanes that
//     share the lane half (one k offset) and hold 16 rows that are distinct mod 16, a row starts at 16-byte slot 5 * row, and 5 is odd, so
//     the 16 reads of a group land in 16 different slots of the 256-byte bank line: conflict free.
//   * Vector A fetch (VEC): where C1, C2 and both channel pitches are multiples of 4 and the tensors 16-byte aligned, a group of 4 consecutive
//     k is 4 consecutive channels of ONE tap and ONE source, so a thread decodes the tap once and fetches the group with one 16-byte load.
//     The general form fetches 2 consecutive k with two 4-byte loads and decodes each (init_conv; ps_conv3d_prec with any channel counts).
//   * The K loop holds no integer division: a thread decodes its k once and steps (channel, tap x, tap y, tap z) by the chunk, and the
//     up-sampling's coordinate / up is a multiplication (div_by).  Loads are unconditional (a padding tap reads voxel 0 and is dropped).
//   * A wave owns 32 rows and all NT column tiles (the 64-row form keeps two of its four waves for the fetch alone: it runs where the whole
//     output has fewer than 2048 voxels).
#include <cstdint>

#include "conv3d_kit.h"

namespace ps {

namespace {

// GRAD: the data gradient (saliency.h's grad fields) -- the row's corner (conv3d_kit.h's conv_row), the fetch's coordinate
// step and the epilogue's column split are the whole difference: the forward walks corner + tap * dil, the gradient gathers from
// (row + pad - tap * dil) / stride where that is whole.
template <int P, int RT, int NT, bool VEC, bool GRAD>
__global__ __launch_bounds__(256) void conv3d_b_kernel(Conv3dArgs a)
{
    constexpr int M = 64 * RT, N = 32 * NT;
    constexpr int KW = VEC ? 4 : 2;    // consecutive k a thread fetches for one row
    constexpr int CG = kBKC / KW;      // such groups in a chunk
    constexpr int RS = 256 / CG;       // rows between a thread's fetches
    constexpr int AI = M / RS;         // rows per thread and chunk
    constexpr int RPC = 8 / KW;        // rows that share one b3_split8
    constexpr int BK = kBKC * N / 256;  // consecutive k of one column per thread: 4 or 8
    static_assert(AI % RPC == 0, "a split takes 8 values");
    __shared__ __attribute__((aligned(16))) unsigned As[P][M * kPW];
    __shared__ __attribute__((aligned(16))) unsigned Bs[P][N * kPW];
    __shared__ int4 rows[M];  // conv_row: the input corner of the row's receptive field (GRAD: the row's voxel + pad) and whether the row exists

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.z, n0 = blockIdx.y * N, m0 = blockIdx.x * M;
    const int Vo = a.Do * a.Ho * a.Wo;
    for (int r = t; r < M; r += 256) rows[r] = conv_row<GRAD>(a, m0 + r, Vo);
    __syncthreads();

    const int cin = a.C1 + a.C2;
    const int Ktot = a.kd * a.kh * a.kw * cin;
    const int nchunks = (Ktot + kBKC - 1) / kBKC;
    const int acg = t % CG, arow = t / CG;
    const int bcol = t % N, bk0 = (t / N) * BK;
    const size_t xs = (size_t)a.Ds * a.Hs * a.Ws;  // voxels of one source sample
    const float* xb = a.x + (size_t)b * xs * a.ldx;
    const float* x2b = a.x2 ? a.x2 + (size_t)b * xs * a.ldx2 : nullptr;
    const float* wb = a.w + (size_t)b * a.w_bstride;

    float areg[AI][KW], breg[BK];
    // Where the thread's k stands: (channel, tap x, tap y, tap z) of each of its KT = KW / NV fetches, decoded ONCE and then stepped by
    // the chunk -- k += 32 carries through the channel and the tap extents, at most one carry per tap of the kernel over the whole walk --
    // so the K loop holds no integer division.  k is behind K exactly when tap z has reached kd.
    constexpr int NV = VEC ? 4 : 1, KT = KW / NV;
    int kci[KT], ktx[KT], kty[KT], ktz[KT];
#pragma unroll
    for (int e = 0; e < KT; ++e) {
        const int k = acg * KW + e, tap = k / cin;
        kci[e] = k - tap * cin, ktx[e] = tap % a.kw, kty[e] = tap / a.kw % a.kh, ktz[e] = tap / (a.kw * a.kh);
    }
    const unsigned upm = div_magic(a.up);  // (used where up > 1)
    const int ldw = GRAD ? a.ldw : a.cout;
    const int sm1 = a.stride - 1;
    const float* wp = wb + (size_t)bk0 * ldw + n0 + bcol;  // the thread's weights of the chunk to fetch
    const bool bin = n0 + bcol < a.cout;
    int kb = bk0;
    auto fetch = [&]() {
#pragma unroll
        for (int e = 0; e < KT; ++e) {
            const bool kin = ktz[e] < a.kd;
            const int dx = ktx[e] * a.dil, dy = kty[e] * a.dil, dz = ktz[e] * a.dil;
            const bool second = kci[e] >= a.C1;
            const float* src = second ? x2b + (kci[e] - a.C1) : xb + kci[e];
            const unsigned ld = second ? a.ldx2 : a.ldx;
#pragma unroll
            for (int i = 0; i < AI; ++i) {
                // (sm1 = stride - 1 and the stride is 1 or 2: % stride is & sm1, / stride is >> sm1)
                const int4 ri = rows[arow + RS * i];
                int z, y, x;
                bool ok = kin && ri.w;
                if constexpr (GRAD) {
                    z = ri.x - dz, y = ri.y - dy, x = ri.z - dx;  // o * stride
                    ok = ok && (z | y | x) >= 0 && ((z | y | x) & sm1) == 0;
                    z >>= sm1, y >>= sm1, x >>= sm1;
                    ok = ok && z < a.D && y < a.H && x < a.W;
                } else {
                    z = ri.x + dz, y = ri.y + dy, x = ri.z + dx;
                    ok = ok && (unsigned)z < (unsigned)a.D && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
                }
                if (!ok) z = y = x = 0;
                if (!GRAD && a.up > 1) z = div_by(z, a.up, upm), y = div_by(y, a.up, upm), x = div_by(x, a.up, upm);
                const float* p = src + (unsigned)((z * a.Hs + y) * a.Ws + x) * ld;  // (a source sample has fewer than 2^31 elements)
                // (the load is unconditional: without `ok` it reads the sample's voxel 0, which exists, and is dropped)
                if constexpr (VEC) {
                    const float4 v = *reinterpret_cast<const float4*>(p);
                    areg[i][0] = ok ? v.x : 0.f, areg[i][1] = ok ? v.y : 0.f, areg[i][2] = ok ? v.z : 0.f, areg[i][3] = ok ? v.w : 0.f;
                } else {
                    const float v = *p;
                    areg[i][e] = ok ? v : 0.f;
                }
            }
            kci[e] += kBKC;
            while (kci[e] >= cin) {
                kci[e] -= cin;
                if (++ktx[e] == a.kw) {
                    ktx[e] = 0;
                    if (++kty[e] == a.kh) kty[e] = 0, ++ktz[e];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < BK; ++i) breg[i] = (bin && kb + i < Ktot) ? wp[(size_t)i * ldw] : 0.f;
        wp += (size_t)kBKC * ldw;
        kb += kBKC;
    };
    // split or round the fetched chunk into the planes
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < AI; i += RPC) {
            float v[8];
#pragma unroll
            for (int r = 0; r < RPC; ++r)
#pragma unroll
                for (int e = 0; e < KW; ++e) v[r * KW + e] = areg[i + r][e];
            const BPlanes<P> p = b3_split8<P>(v);
#pragma unroll
            for (int pl = 0; pl < P; ++pl) {
                const unsigned w[4] = {p.p[pl].x, p.p[pl].y, p.p[pl].z, p.p[pl].w};
#pragma unroll
                for (int r = 0; r < RPC; ++r) {
                    unsigned* dst = &As[pl][(arow + RS * (i + r)) * kPW + acg * (KW / 2)];
                    if constexpr (VEC) *reinterpret_cast<uint2*>(dst) = make_uint2(w[2 * r], w[2 * r + 1]);
                    else *dst = w[r];
                }
            }
        }
        stage_b<P, BK>(breg, &Bs[0][bcol * kPW + bk0 / 2], N * kPW);
    };

    f32x16 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    const int c32 = lane & 31, hl = lane >> 5;
    const bool mma = wave * 32 < M;  // (wave uniform)
    const int fa = (wave * 32 + c32) * kPW + hl * 4, fb = c32 * kPW + hl * 4;
    fetch();
#pragma unroll 1
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        stage();
        __syncthreads();
        if (chunk + 1 < nchunks) fetch();
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

    float* yb = a.y + (size_t)b * Vo * a.ldy;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = n0 + j * 32 + c32;
        if (col >= a.cout) continue;
        if constexpr (GRAD) {
            const bool first = col < a.nsplit;
            float* o = first ? yb + col : a.y2 + (size_t)b * Vo * a.ldy2 + (col - a.nsplit);
            const int ld = first ? a.ldy : a.ldy2;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int v = c_row_b(m0 + wave * 32, r, hl);
                if (v < Vo) o[(size_t)v * ld] = acc[j][r];
            }
        } else {
            const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int v = c_row_b(m0 + wave * 32, r, hl);
                if (v < Vo) yb[(size_t)v * a.ldy + col] = acc[j][r] + bias;
            }
        }
    }
}

template <int P, int RT, int NT>
void launch(hipStream_t sm, const Conv3dArgs& a, bool vec)
{
    const int Vo = a.Do * a.Ho * a.Wo;
    const dim3 grid((unsigned)ceil_div(Vo, 64 * RT), (unsigned)ceil_div(a.cout, 32 * NT), (unsigned)a.B);
    if (a.grad) {
        // (the split data gradient exists with the 16-byte fetch alone: conv3d_train.hip routes the other to the fp32 kernel)
        if (vec) hipLaunchKernelGGL((conv3d_b_kernel<P, RT, NT, true, true>), grid, dim3(256), 0, sm, a);
        else if constexpr (P == 1) hipLaunchKernelGGL((conv3d_b_kernel<P, RT, NT, false, true>), grid, dim3(256), 0, sm, a);
    } else if (vec) hipLaunchKernelGGL((conv3d_b_kernel<P, RT, NT, true, false>), grid, dim3(256), 0, sm, a);
    else hipLaunchKernelGGL((conv3d_b_kernel<P, RT, NT, false, false>), grid, dim3(256), 0, sm, a);
}

// (conv3d_kit.h's form rule)
template <int P>
void launch_p(hipStream_t sm, const Conv3dArgs& a)
{
    const bool vec = conv3d_b_vec(a);
    conv_form_b((int64_t)a.Do * a.Ho * a.Wo >= 2048, a.cout, [&](auto rt, auto nt) { launch<P, decltype(rt)::value, decltype(nt)::value>(sm, a, vec); });
}

}  // namespace

bool conv3d_b_vec(const Conv3dArgs& a)
{
    return a.C1 % 4 == 0 && a.C2 % 4 == 0 && a.ldx % 4 == 0 && (a.C2 == 0 || a.ldx2 % 4 == 0)
           && ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.x2)) & 15) == 0;
}

void conv3d_b_launch(hipStream_t sm, const Conv3dArgs& a)
{
    if (a.precision == PS_PREC_BF16) launch_p<1>(sm, a);
    else launch_p<3>(sm, a);
}

}  // namespace ps
