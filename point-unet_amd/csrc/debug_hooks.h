/* debug_hooks.h -- C declarations of the TEST-ONLY library point-unet_amd/libpointseg_debug.so (csrc/debug_hooks.hip).
 * Not part of the product ABI (include/pointseg.h) and not in the product library: the doors below let the test-suite run the
 * product's own host logic (kd-tree construction rules, the per-query search routine the HIP kernel instantiates, the MFMA weight
 * packing) without a GPU, and read a device-built tree back array for array.  The library links against libpointseg_hip.so. */
#ifndef POINTSEG_DEBUG_H
#define POINTSEG_DEBUG_H
#include "../../include/pointseg.h"
#ifdef __cplusplus
extern "C" {
#endif
/* The product's own kd-tree construction + the per-query search routine the HIP kernel instantiates, run on the
 * host.  K in {1,5,7,16,32}. */
int ps_debug_knn_host(const float* support, const float* queries, int64_t B, int64_t n_support,
                      int64_t n_queries, int64_t K, int32_t* out_idx);
/* vind i32[n], nodes i32[2n,4], pts f32[n,4], root_depth i32[2], bbox f32[6] (layout: csrc/kdtree.h). */
int ps_debug_kdtree_host(const float* support, int64_t n, int32_t* vind, int32_t* nodes, float* pts,
                         int32_t* root_depth, float* bbox);
/* The same arrays from the DEVICE builder (csrc/kdtree_build.hip); needs a GPU.  Unreached node slots are
 * unspecified: compare by walking from the root. */
int ps_debug_kdtree_device(ps_context* ctx, const float* support, int64_t n, int32_t* vind, int32_t* nodes,
                           float* pts, int32_t* root_depth, float* bbox);
/* MFMA B-fragment packing of a row-major W[cin,cout] (csrc/rowgemm.h). */
int ps_debug_pack_weights(const float* W, int cin, int cout, int ntb, float* out);
/* Three-plane bfloat16 image of a row-major W[cin,cout] for the split-bf16 attention kernels (csrc/attpool32b.hip: pack_b3):
 * out = uint16 [cout/32][cin/16][3 planes][64 lanes][8]. */
int ps_debug_pack_b3(const float* W, int cin, int cout, uint16_t* out);
/* One dense layer of the deep levels, Y = act([X1[g1] | X2[g2]] . W + b), through gemm32b.hip (split_bf16 != 0: bf16 MFMA over exact
 * three-way splits) or gemm32.hip (fp32 MFMA); needs a GPU.  x1 / x2 / g1 / g2 / y: DEVICE pointers (g* may be NULL: plain rows; gm / gn:
 * batched gather, row r reads x[(r / gm) * gn + g[r]] when gm != 0), W [c1 + c2, cout] and bias [cout]: HOST.  Returns PS_EINVAL when the
 * shape does not fit the kernel. */
int ps_debug_gemm32(ps_context* ctx, int split_bf16, const float* x1, int ld1, int c1, const int32_t* g1, const float* x2, int ld2, int c2,
                    const int32_t* g2, int gm, int gn, const float* W, const float* bias, int64_t R, int cout, int leaky, float* y, int ldy);
/* The launch ps_debug_gemm32 (and the network's own dense layers) make on this context for R x cin x cout: out4 = {rw, cw, sk, pd} -- rw x cw
 * blocks of 32 x 32 per wave, sk waves splitting the K axis (chunks of 8 inputs for the fp32 kernel, 16 for the split form) into slices
 * [nq k / sk, nq (k + 1) / sk), pd chunks in flight.  Host only: no GPU work. */
int ps_debug_gemm32_plan(ps_context* ctx, int split_bf16, int64_t R, int cin, int cout, int* out4);

/* The experiment knobs of one context (csrc/common.h, struct ps::Tuning), by C++ field name ("inv_bucket", "gemm32b_rw", ...).  Set accepts
 * exactly the values the kernels are compiled for (the rules of the -DPS_TUNING_ENV build, without its clamping) and refuses anything else,
 * and unknown names, with PS_EINVAL.  Kernel dispatch reads the knobs per call; the native trainer reads its train_* knobs (and
 * convbn_max_c / convbn_rect_max per step, from the same context) -- set them BEFORE ps_trainer_create. */
int ps_debug_set_tuning(ps_context* ctx, const char* field, double value);
int ps_debug_get_tuning(ps_context* ctx, const char* field, double* value);
/* The field names the two doors above know, '\n'-separated and NUL-terminated, into buf[cap]; PS_EINVAL when cap is too small.  No context. */
int ps_debug_tuning_fields(char* buf, int cap);
/* sizeof(ps_volume_sample_args) as the library was compiled: the ctypes mirror (point-unet_amd/_lib.py) is checked against it. */
int ps_debug_volume_sample_args_size(void);

#ifdef __cplusplus
}
#endif
#endif /* POINTSEG_DEBUG_H */
