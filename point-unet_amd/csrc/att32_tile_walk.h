// att32_tile_walk.h -- text of att32_tile.h: the tile walk, included once in front of the tile loop `for (int t0 = t_first; t0 < t_end;
// t0 += t_step)`, with the kernel argument `a`, `KN`, `PPT`, `c32` and the workgroup's share in scope: `TPW` tiles per workgroup, of
// which this wave works on tile `tiw` (WAVES / wave for a wave per tile, 1 / 0 for the waves that share one).
//
// Tiles walk a contiguous EIGHTH of the points per XCD, PPT consecutive points per tile: workgroups go to the 8 XCDs round-robin, and with
// `order` the t-th point is the t-th in kd-tree leaf order, so an XCD's neighbour gathers mostly hit its own L2 (the PointWalk of
// attpool.hip, here in units of tiles).
//
// Within an XCD the tiles are dealt WAVE-major: tile `tiw * slots + slot + j * slots * TPW` of the eighth goes to wave `tiw` of workgroup
// `slot`.  The last round is partial (level 1: 2 813 tiles over 512 or 384 waves), and its tiles so go to wave 0 of every workgroup, then
// wave 1 of every workgroup, ...: every CU takes the same share of the remainder, on its low waves.  Dealt slot-major (`slot * TPW + tiw`)
// the remainder filled ALL waves of the low workgroups, whose SIMDs ran 24 tiles against the others' 20-21, and the launch lasts as long
// as its busiest SIMD.  ASSUMED, not read from a counter: a workgroup's waves go to the CU's four SIMDs round-robin (wave w on SIMD w & 3),
// so consecutive low waves are different SIMDs and the remainder is even over SIMDs too (22 tiles each at level 1).  Measured: the
// d = 64 att32b launches 5-6 % shorter (8.3 % if tiles per SIMD were all), d = 128 (6 tiles on the busiest SIMD either way) unchanged
// (DESIGN 4.2).  With TPW = 1 both deals are the same walk.
const int per_xcd = ((((a.n_total + 7) >> 3) + PPT - 1) / PPT) * PPT;
const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;  // the host launches a multiple of 8
const int t_end = min(a.n_total, (xcd + 1) * per_xcd);
const int t_first = xcd * per_xcd + (tiw * slots + slot) * PPT, t_step = slots * TPW * PPT;
// Geometry of a tile = three dependent gathers (leaf order -> neighbour index -> coordinates): the NEXT tile's chain is issued in pieces
// between the phases of the current tile (gstage 0..2, placed by each kernel), so none of its latency is exposed.
int n_pp[PPT], n_nl = 0;
float n_c[3], n_n[3];
// (att32_kernel is VALU-issue bound at d <= 128 -- one VALU instruction per SIMD every four cycles --, so the index arithmetic is kept
//  lean: no integer division for a single cloud, 24-bit multiplies, 32-bit element offsets from uniform bases)
const bool one_cloud = a.n_total == a.n_cloud;
auto cloud_base = [&](int row) { return one_cloud ? 0 : (row / a.n_cloud) * a.n_cloud; };
auto gstage = [&](int st, int t0n) {
    if (t0n >= t_end) return;
    if (st == 0) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int t = min(t0n + i, t_end - 1);
            n_pp[i] = a.order ? cloud_base(t) + a.order[t] : t;
        }
    } else if (st == 1) {
        const unsigned p = PPT == 2 ? (c32 >= KN ? n_pp[PPT - 1] : n_pp[0]) : n_pp[0];
        n_nl = a.idx[p * (unsigned)KN + (unsigned)(c32 & (KN - 1))];
        const float* cp = a.xyz + 3u * p;
        n_c[0] = cp[0]; n_c[1] = cp[1]; n_c[2] = cp[2];
    } else {
        const int p = PPT == 2 ? (c32 >= KN ? n_pp[PPT - 1] : n_pp[0]) : n_pp[0];
        n_nl += cloud_base(p);
        const float* np = a.xyz + 3u * (unsigned)n_nl;
        n_n[0] = np[0]; n_n[1] = np[1]; n_n[2] = np[2];
    }
};
gstage(0, t_first);
gstage(1, t_first);
gstage(2, t_first);
