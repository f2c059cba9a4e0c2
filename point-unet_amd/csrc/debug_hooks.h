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
 * host.  K: every size the kernels are compiled for (PS_KNN_KS, csrc/kdtree.h); any other returns PS_EINVAL, out_idx untouched. */
int ps_debug_knn_host(const float* support, const float* queries, int64_t B, int64_t n_support,
                      int64_t n_queries, int64_t K, int32_t* out_idx);
/* vind i32[n], nodes i32[2n,4], pts f32[n,4], root_depth i32[2], bbox f32[6] (layout: csrc/kdtree.h). */
int ps_debug_kdtree_host(const float* support, int64_t n, int32_t* vind, int32_t* nodes, float* pts,
                         int32_t* root_depth, float* bbox);
/* The same arrays from the DEVICE builder (csrc/kdtree_build.hip); needs a GPU.  Unreached node slots are
 * unspecified: compare by walking from the root. */
int ps_debug_kdtree_device(ps_context* ctx, const float* support, int64_t n, int32_t* vind, int32_t* nodes,
                           float* pts, int32_t* root_depth, float* bbox);
/* T trees built as ONE set, the way the product builds them (one TreeSetPlan, one build_trees); needs a GPU.  support: the trees' rows one
 * after the other, f32 [sum n, 3]; n: i32 [T], every n[i] >= 1.  Every output is the tree-by-tree concatenation of what
 * ps_debug_kdtree_device returns for one tree: vind i32 [sum n], nodes i32 [2 sum n, 4], pts f32 [sum n, 4], root_depth i32 [T, 2],
 * bbox f32 [T, 6]; and with them fat i32 [6 sum n, 4], the three-record image the searches read (TreeView::fat: records 3 id .. 3 id + 2 =
 * node id, its first child, its second child, a leaf child as zeros; only odd ids are written), and copy f32 [sum of n[i] with
 * want_copy[i] != 0, 3]: the rows TreeSetPlan::copy_dst received, for those trees in order (want_copy i32 [T], or NULL: none).
 * stats i32 [PS_DEBUG_KDTREE_STATS]: the counters of the plan's head block after the build.  "Node" = a node of a finished tree, root
 * at depth 0; its size = its points; L = stats[0]; kHuge = kMid, kChunk, kSmall, kHugeLevels = 8: csrc/kdtree_build.hip.
 *   [0]       chunked levels launched: min(kHugeLevels, the smallest L with (max n >> L) <= kMid), ONE value for the whole set
 *   [1 + l]   l = 0..7: HugeState::ntasks[l] = nodes of all trees at depth l with more than kHuge points, for l < L; 0 from L on (route_task
 *             is the only writer, and every ancestor of such a node is a chunked task itself)
 *   [9 + l]   l = 0..7: HugeState::nchunks[l] = sum of ceil(size / kChunk) over the nodes counted in [1 + l]; 0 from L on
 *   [17]      QueueCounters::level[L], the queue build_level_kernel starts from = nodes at depth L with more than kMid points (their
 *             parents are chunked tasks of level L - 1; the kernel itself parks what it meets below on a stack in LDS and counts nothing)
 *   [18]      QueueCounters::mid, pushes to the mid queue = nodes of kSmall + 1 .. kMid points that are roots or whose parent has
 *             more than kMid points (build_mid_kernel keeps its own children above kSmall in LDS)
 *   [19]      QueueCounters::small, pushes to the small queue = nodes of at most kSmall points, leaves included, that are roots or
 *             whose parent has more than kSmall points
 *   [20] [21] the status words (BuildFlag, csrc/kdtree_build.h): kFlagStackOverflow (written by searches only: 0 after a build),
 *             kFlagQueueOverflow (a builder queue overflowed); this door does not refuse on it */
#define PS_DEBUG_KDTREE_STATS 22
int ps_debug_kdtree_device_set(ps_context* ctx, const float* support, const int32_t* n, int64_t T, const int32_t* want_copy, int32_t* vind,
                               int32_t* nodes, float* pts, int32_t* fat, int32_t* root_depth, float* bbox, float* copy, int32_t* stats);
/* MFMA B-fragment packing of a row-major W[cin,cout] (csrc/rowgemm.h). */
int ps_debug_pack_weights(const float* W, int cin, int cout, int ntb, float* out);
/* Three-plane bfloat16 image of a row-major W[cin,cout] for the split-bf16 attention kernels (csrc/attpool32b.hip: pack_b3):
 * out = uint16 [cout/32][cin/16][3 planes][64 lanes][8]. */
int ps_debug_pack_b3(const float* W, int cin, int cout, uint16_t* out);
/* The three planes of the same W by the DEVICE split (csrc/b3_ops.h: b3_split8, through the training step's packing kernel, kind 5 =
 * the K order of pack_b3); needs a GPU.  W, out: DEVICE pointers; out = uint16 [cin/16][cout/32][3 planes][64 lanes][8]. */
int ps_debug_pack_b3_device(ps_context* ctx, const float* W, int cin, int cout, void* out);
/* One dense layer of the deep levels, Y = act([X1[g1] | X2[g2]] . W + b), through gemm32b.hip (split_bf16 != 0: bf16 MFMA over exact
 * three-way splits) or gemm32.hip (fp32 MFMA); needs a GPU.  x1 / x2 / g1 / g2 / y: DEVICE pointers (g* may be NULL: plain rows; gm / gn:
 * batched gather, row r reads x[(r / gm) * gn + g[r]] when gm != 0), W [c1 + c2, cout] and bias [cout]: HOST.  Returns PS_EINVAL when the
 * shape does not fit the kernel.  split_bf16 = 2: the ONE-plane form of gemm32b.hip -- both operands rounded once to bfloat16 (round to nearest
 * even), fp32 accumulation: a layer of a network at PS_PREC_BF16 (include/pointseg_forward_precision.h). */
int ps_debug_gemm32(ps_context* ctx, int split_bf16, const float* x1, int ld1, int c1, const int32_t* g1, const float* x2, int ld2, int c2,
                    const int32_t* g2, int gm, int gn, const float* W, const float* bias, int64_t R, int cout, int leaky, float* y, int ldy);
/* The launch ps_debug_gemm32 (and the network's own dense layers) make on this context for R x cin x cout: out4 = {rw, cw, sk, pd} -- rw x cw
 * blocks of 32 x 32 per wave, sk waves splitting the K axis (chunks of 8 inputs for the fp32 kernel, 16 for the split form) into slices
 * [nq k / sk, nq (k + 1) / sk), pd chunks in flight (split_bf16 = 2: the one-plane form -- the same tiles and slices, its own ring depth).  Host
 * only: no GPU work. */
int ps_debug_gemm32_plan(ps_context* ctx, int split_bf16, int64_t R, int cin, int cout, int* out4);

/* A chain of 1..4 dense layers over R rows, act_l = act([act_{l-1} | extra_l] . W_l + b_l), act_{-1} = [x1[g1] | x2[g2]] (csrc/rowgemm.h: rowchain).
 * W [cin, cout] and bias [cout] (NULL: zeros): HOST.  x1 / x2 / g1 / g2 / y / extra: DEVICE pointers (NULL: absent; g*m / g*n: batched gather, row r
 * reads x[(r / gm) * gn + g[r]] when gm != 0).  y: optional store of the layer's rows, row stride ldy.  extra (layers > 0): plain rows of c_extra
 * channels appended after the previous activations; extra_gather only exists to be refused. */
typedef struct ps_debug_chain_layer {
    const float* W;
    const float* bias;
    int cin, cout, leaky;
    float* y;
    int ldy;
    const float* extra;
    int ld_extra, c_extra;
    const int32_t* extra_gather;
} ps_debug_chain_layer;
typedef struct ps_debug_chain_desc {
    int n_layers;
    ps_debug_chain_layer layer[4];
    const float* x1; const int32_t* g1; int ld1, c1, g1m, g1n;
    const float* x2; const int32_t* g2; int ld2, c2, g2m, g2n;
    int64_t R;
} ps_debug_chain_desc;
/* Runs the chain with freshly packed weights (pack_weights + zero-padded bias, and the k-permuted image when cin % 16 == 0, as ps_randla_set_weights
 * packs every layer); needs a GPU.  form 0: rowchain() as the network calls it, with a weight-image cache; 1: regchain with the image re-ordered
 * inside the kernel (no cache); 2: rowchain_lds (the LDS-staged kernel); 3: layer by layer through rowgemm (16x16x4 kernels; un-stored rows go to
 * scratch).  Returns PS_EINVAL, with a message, when the chain does not fit the form.
 * forms 4..7 = forms 0..3 on the images of a network at PS_PREC_BF16 (include/pointseg_forward_precision.h): every layer whose cin is a multiple
 * of 16 and at least 32 has both operands rounded once to bfloat16 -- its images hold the rounded weights and the kernel that takes it rounds the
 * activations as it loads them; the other layers are what they are in forms 0..3.  Form 5 (regchain) takes a chain only when EVERY layer is
 * rounded and the shape is one of the one-plane policy's; a mixed chain runs on forms 4 (which then picks rowchain_kernel), 6 and 7. */
int ps_debug_chain(ps_context* ctx, const ps_debug_chain_desc* d, int form);
/* The launch rowchain() makes for the same description: out4 = {form (0: the chain fits neither kernel, 1: regchain_kernel, 2: rowchain_kernel),
 * workgroups, dynamic LDS bytes, rowchain_kernel's float4 input staging (log2 of the float4s per row; 0 = scalar staging)}.  A workgroup is four
 * waves that each take one 16-row tile per round: past workgroups * 64 rows a wave walks to a second tile.  Host only: reads the channel counts
 * and the alignment of the pointers, never what they point to; W / bias may be NULL. */
int ps_debug_chain_plan(const ps_debug_chain_desc* d, int* out4);
/* The same at a precision of include/pointseg_forward_precision.h: 1 (PS_PREC_BF16X3) = ps_debug_chain_plan, 2 (PS_PREC_BF16) = the launch of
 * ps_debug_chain's form 4, where form 3 = regchain_kernel on one plane of rounded operands (every layer rounded: eight waves per workgroup, 2
 * bytes per weight of LDS) and form 2 = rowchain_kernel, which rounds layer by layer. */
int ps_debug_chain_plan_prec(const ps_debug_chain_desc* d, int precision, int* out4);
/* The operand policy of regchain's routed chain shapes on this context (on by default): 1 = bf16 MFMA over exact three-way splits, 0 = the fp32
 * MFMA for every shape.  ps_debug_chain forms 0 and 1 follow it; ps_debug_chain_plan has no context and reports the fp32 launch. */
int ps_debug_set_regchain_b3(ps_context* ctx, int on);
/* Where att_pool_stage sends a d = 16 / K = 16 stage of the direct formulation on this context (on by default): 1 = att_lane_kernel
 * (attpool_lane.hip, the vector ALU), 0 = att_direct_kernel (16x16x4 MFMA).  ps_debug_att_stage form 0 and ps_debug_att_form follow it. */
int ps_debug_set_att_lane(ps_context* ctx, int on);
/* One attentive-pooling stage (1 or 2) of encoder level `level` of a live network with its weights set, on the network's own packed images
 * (log2(e) scaling and weight halves included); AttStage is filled as ps_randla_forward fills it.  xyz f32[n_total, 3], idx i32[n_total, K]
 * (cloud-local), order i32[n_total] or NULL, fg f32[n_total, d/2 + d] = [f | G] for d >= 64 and f32[n_total, d/2] = f below, agg f32[n_total, d]:
 * DEVICE pointers.  form 0: att_pool_stage (the product's dispatch), 1: att_pool32b_stage (split-bf16 32x32), 2: att_pool32_stage (fp32 32x32),
 * 3: att_pool16_stage (16x16x4: the direct kernel at d <= 32, att_kernel above), 4: att_lane_stage (the vector-ALU kernel of attpool_lane.hip,
 * d = 16 and K = 16 only, whatever the context's att_lane switch says), 5: att_pool32b_stage on ONE plane of rounded operands (LFA mlp2 and the
 * score product; LocSE stays on the exact split), on the network's PS_PREC_BF16 images whatever its precision -- PS_EINVAL where form 1 is.  Form 0
 * follows the network's precision.  PS_EINVAL when the level does not fit the form. */
int ps_debug_att_stage(ps_randla* net, int level, int stage, int form, const float* xyz, const int32_t* idx, const int32_t* order, const float* fg,
                       int64_t n_total, int64_t n_cloud, float* agg);
/* The form (1 .. 5, numbered as above; 5 only for a network at PS_PREC_BF16) att_pool_stage takes for stage 1 or 2 of encoder level `level` at k neighbours and n_total rows, on the
 * network's context as its knobs stand -- bit-identical outputs cannot show which kernel ran.  Host only.  Returns the form, not a status: -1 on
 * a bad argument. */
int ps_debug_att_form(ps_randla* net, int level, int stage, int k, int64_t n_total);
/* The kernel family rowgemm() takes, on the network's context and at the network's precision, for one of the network's OWN dense layers over R
 * rows: which 0 = att_pooling_1 mlp of encoder level `level`, 1 = its att_pooling_2 mlp, 2 = its [mlp2 ; shortcut], 3 = decoder_0, 4 = decoder step
 * `level`.  Returns 5 = gemm32b on one plane of rounded operands, 1 = gemm32b on the exact split, 2 = gemm32, 3 = the 16x16 kernels of rowgemm.hip;
 * -1 on a bad argument.  Host only. */
int ps_debug_dense_form(ps_randla* net, int which, int level, int64_t R);
/* Points one pass of att_lane_kernel's largest grid covers (workgroups x waves x points per wave iteration): past it a wave walks on. */
int ps_debug_att_lane_pass_points(void);

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

/* The shared scan and radix sort (csrc/sortscan.h) and the partial-sum reducer (csrc/reduce_partials.h) on their own.
 * Host only, no context: the values of scan_workspace_words(n), sort_workspace_words(n) (unsigned words), scan_launches(n) and
 * radix_sort_pairs_launches(n, bits).  These return a value, not a status: a negative n (or bits outside 1..64) gives -1. */
int64_t ps_debug_scan_words(int64_t n);
int64_t ps_debug_sort_words(int64_t n);
int ps_debug_scan_launches(int64_t n);
int ps_debug_sort_launches(int64_t n, int bits);
/* exclusive_scan_u32 on the context's stream, then a synchronise; needs a GPU.  in / out: DEVICE u32 [n] (in == out is allowed; any 4-byte
 * alignment), work: the CALLER's device buffer of at least ps_debug_scan_words(n) words -- the door allocates nothing, so a test can put guard
 * bands around it. */
int ps_debug_scan_u32(ps_context* ctx, const uint32_t* in, uint32_t* out, int64_t n, uint32_t* work);
/* radix_sort_pairs_u32 (key_bytes 4) / radix_sort_pairs_u64 (key_bytes 8; anything else is PS_EINVAL, as are bits outside 1..8 key_bytes) on the
 * context's stream; needs a GPU.  k0 / k1: DEVICE keys [n] of key_bytes each, every key below 2^bits; v0 / v1: DEVICE u32 [n]; (k0, v0) is the
 * input and is overwritten; work: the caller's DEVICE buffer of at least ps_debug_sort_words(n) words.  *which_out (HOST) = 0 / 1: the pair of
 * arrays that holds the sorted result; written before the synchronise. */
int ps_debug_sort_pairs(ps_context* ctx, int key_bytes, void* k0, void* k1, uint32_t* v0, uint32_t* v1, int64_t n, int bits, uint32_t* work,
                        int* which_out);
/* out[i] = sum over b of part[b * nv + i] through the kernels of csrc/reduce_partials.h on the grid every caller uses, ceil(nv / 16) workgroups
 * of 256, then a synchronise; needs a GPU.  form 0: reduce_partials_kernel<float>, 1: reduce_partials_kernel<double>, 2: reduce_partials2_kernel<float>,
 * 3: reduce_partials2_kernel<float, double> (float partials added in double).  part: DEVICE [n_part, nv] of the form's type; forms 0 / 1 write
 * out0 [nv] (n0 and out1 are ignored); forms 2 / 3 write values [0, n0) to out0 and [n0, nv) to out1, 0 <= n0 <= nv.  The reducer is a header of
 * templates, so the product library has no symbol to call: this door instantiates the templates from the shared header -- the same text as the
 * product's kernels, compiled a second time. */
int ps_debug_reduce_partials(ps_context* ctx, int form, const void* part, int n_part, int nv, int n0, void* out0, void* out1);

#ifdef __cplusplus
}
#endif
#endif /* POINTSEG_DEBUG_H */
