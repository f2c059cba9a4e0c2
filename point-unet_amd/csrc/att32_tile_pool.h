// att32_tile_pool.h -- text of att32_tile.h: attentive pooling of one 32-column block `cb` of a tile, included in a block that has in
// scope: `acc` (f32x16) the product f_xyz . Wfc[H:, :] of the block (C[row][channel]: register r of this lane = row (r & 3) + 8 (r >> 2)
// + 4 hl, column c32), `gs` (f32x2[8]) the gathered G values and `vv` (f32x2[8]) the gathered f values of the same rows (filled here
// for the columns >= H, whose values are f_xyz), `TX` the fp32 LDS tile of f_xyz, and the tile's `pp`, `t0`, `t_end`.
// scores = G[nbr] + acc, softmax over the K rows of a point, weighted sum of the values -> agg[point][32 cb + c32]
if (cb * 32 >= H) {  // values = f_xyz (LDS tile)
    const float* tv = TX + (cb * 32 - H + c32) + 4 * hl * PITCH;
#pragma unroll
    for (int r = 0; r < 16; ++r) vv[r >> 1][r & 1] = tv[((r & 3) + 8 * (r >> 2)) * PITCH];
}
// the Wfc[H:, :] image is pre-multiplied by log2(e) (pack calls in randla.hip), the gathered G joins with the same factor:
// softmax(s) = exp2(s' - max s') with s' = s log2(e) -- one multiply per score less than expf
f32x2 sc[8];  // register pairs: the arithmetic runs on v_pk_*_f32 (two scores per instruction)
const f32x2 l2e = {1.4426950408889634f, 1.4426950408889634f};
#pragma unroll
for (int j = 0; j < 8; ++j) sc[j] = __builtin_elementwise_fma(gs[j], l2e, f32x2{acc[2 * j], acc[2 * j + 1]});
constexpr int PP = 8 / PPT;  // register pairs per point: a channel's K scores sit in 8 (16) registers of the lanes l and l ^ 32
#pragma unroll
for (int pi = 0; pi < PPT; ++pi) {
    float m = fmaxf(sc[pi * PP][0], sc[pi * PP][1]);
#pragma unroll
    for (int j = 1; j < PP; ++j) m = fmaxf(m, fmaxf(sc[pi * PP + j][0], sc[pi * PP + j][1]));
    m = swap32_max(m);
    const f32x2 mm = {m, m};
    f32x2 ssum2 = {0.f, 0.f}, num2 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < PP; ++j) {
        const f32x2 dd = sc[pi * PP + j] - mm;
        const f32x2 ex = {__builtin_amdgcn_exp2f(dd[0]), __builtin_amdgcn_exp2f(dd[1])};
        ssum2 += ex;
        num2 = __builtin_elementwise_fma(ex, vv[pi * PP + j], num2);
    }
    const float ssum = swap32_sum(ssum2[0] + ssum2[1]);
    const float num = swap32_sum(num2[0] + num2[1]);
    if (hl == 0 && t0 + pi < t_end) a.agg[__umul24(pp[pi], D) + (unsigned)(cb * 32 + c32)] = num * __builtin_amdgcn_rcpf(ssum);
}
