// gemm32_frame.h -- the one kernel frame of the deep dense layers, gemm32.hip (fp32 MFMA) and gemm32b.hip (split-bf16 MFMA):
//
//   Y[r, :] = act([X1[g1[r]] | X2[g2[r]]] . W + b)
//
// A wave owns (32 RW) rows x (32 CW) columns.  The frame owns everything the two forms share: the XCD-aware walk of the workgroup grid,
// the row sources, the register ring of K chunks, the split-K reduction through LDS, bias and epilogue (gemm32_frame_body.h), and on the
// host the argument struct, the `fits` predicate and the RowSrc copy (below).  What a form brings is an operand policy `Op`:
//
//   Op::KC                   inputs per K chunk (8 / 16); a lane half reads KC / 2 consecutive inputs of its row
//   Op::wvec, Op::WV         a chunk's weights per column block: WV 16-byte vectors of type wvec, image [column block][chunk][vector][lane]
//   Op::pd<RW, CW>()         ring depth: chunks in flight ahead of the products
//   Op::products(x, w, acc)  the MFMAs of one chunk: x[RW][KC / 8] float4 of activations, w[CW][WV] weights, acc[RW][CW]
//
// The body is text that the two __global__ functions include, not a __forceinline__ function template.  As a function of its own the
// compiler simplifies it once before it inlines it into a kernel and once more after, and the second pass is not idempotent: measured on
// all 20 instantiations, the template form kept VGPRs, LDS and the instruction mix but moved the scalar register count of every CW = 1
// kernel (kernel-argument loads merged differently, address sums re-associated), by value, by reference or with typed global pointers
// alike.  Included, gemm32b_kernel compiles to the code it had as a file of its own, byte for byte, and gemm32_kernel to the same
// registers, LDS and instruction counts.
#pragma once

#include "mfma_tile.h"
#include "rowgemm.h"

namespace ps {

struct Gemm32Args {
    const float* x1; const int32_t* g1; int ld1, c1, g1m, g1n;
    const float* x2; const int32_t* g2; int ld2, c2, g2m, g2n;
    const void* wp;     // the form's image of W[cin, cout]: pack_p32 (attpool.h) / pack_p32b (rowgemm.h)
    const float* bias;  // [cout]
    float* y;
    int ldy, R, cin, cout, leaky;
    int rgroups, cgroups;  // workgroup grid: row groups x column groups (see the XCD mapping in the frame)
};

// ---- host side -----------------------------------------------------------------------------------------------------------------
// `image`: the layer's weight image of the form (null when not built); kc: the form's K chunk
inline bool gemm32_fits_kc(const void* image, int kc, const PackedLinear& L, const RowSrc& s1, const RowSrc& s2, int64_t R, int ldy)
{
    return image && !L.accum && R <= 32768 && L.cin % kc == 0 && L.cout % 32 == 0 && s1.c % kc == 0 && s2.c % kc == 0 && s1.c + s2.c == L.cin &&
           s1.ld % 4 == 0 && (s2.c == 0 || s2.ld % 4 == 0) && (reinterpret_cast<uintptr_t>(s1.x) & 15) == 0 &&
           (s2.c == 0 || (reinterpret_cast<uintptr_t>(s2.x) & 15) == 0) && ldy > 0;
}

inline Gemm32Args gemm32_args(const void* image, const PackedLinear& L, const RowSrc& s1, const RowSrc& s2, int64_t R, float* y, int ldy, const Gemm32Plan& p)
{
    Gemm32Args a;
    a.x1 = s1.x; a.g1 = s1.gather; a.ld1 = s1.ld; a.c1 = s1.c; a.g1m = s1.gm; a.g1n = s1.gn;
    a.x2 = s2.x; a.g2 = s2.gather; a.ld2 = s2.ld; a.c2 = s2.c; a.g2m = s2.gm; a.g2n = s2.gn;
    a.wp = image; a.bias = L.bias; a.y = y; a.ldy = ldy; a.R = (int)R; a.cin = L.cin; a.cout = L.cout; a.leaky = L.leaky;
    a.rgroups = p.rgroups;
    a.cgroups = p.cgroups;
    return a;
}

}  // namespace ps
