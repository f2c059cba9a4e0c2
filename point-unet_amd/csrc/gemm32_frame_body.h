// gemm32_frame_body.h -- the body of gemm32_kernel<CW, SK> (gemm32.hip) and gemm32b_kernel<RW, CW, SK> (gemm32b.hip).
// No header of declarations: the two __global__ functions include it as their body, with the operand policy `Op`, `RW`, `CW`, `SK` and the
// kernel argument `a` (Gemm32Args) in scope.  gemm32_frame.h says what a policy provides and why this is text and not a function.
//
// waves of a workgroup: SK along K (same output block), 4 / SK consecutive row units of 32 RW rows (SK = 8: eight waves, one row unit -- the
// few-row / long-K layers of levels 3-4 and the decoder, whose launch is one exposed chain of loads and MFMAs per wave: half the chain)
{
    constexpr int KC = Op::KC, XV = KC / 8, WV = Op::WV;
    using wvec = typename Op::wvec;
    constexpr int RU = SK > 4 ? 1 : 4 / SK;  // row units per workgroup
    __shared__ float red[SK > 1 ? RU * (SK - 1) * RW * CW * 16 * 64 : 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hl = lane >> 5, c32 = lane & 31;
    const int kw = wave % SK, ruw = wave / SK;
    // XCD-aware mapping: workgroups go to the 8 XCDs round-robin (block b -> XCD b % 8).  The (column group, row group) space is
    // walked column-group-major and cut into eight contiguous pieces, one per XCD, so an XCD's L2 holds only its own column
    // groups' weight panels (1/8 of W: the 4 MB matrices of the deepest levels do not fit one 4 MB L2 next to the activations)
    // and consecutive workgroups of an XCD reuse the same panel.
    const int total = a.rgroups * a.cgroups, per_xcd = (total + 7) >> 3;
    const int slot = (int)(blockIdx.x >> 3);
    const int u = (int)(blockIdx.x & 7) * per_xcd + slot;
    if (slot >= per_xcd || u >= total) return;
    const int ru = (u % a.rgroups) * RU + ruw;  // row unit: rows [ru * 32 RW, (ru + 1) * 32 RW)
    const int cb = (u / a.rgroups) * CW;        // first 32-column block
    const int nq = a.cin / KC, nq1 = a.c1 / KC;
    const int qa = (nq * kw) / SK, qb = (nq * (kw + 1)) / SK;
    const bool live = ru * 32 * RW < a.R;

    f32x16 acc[RW][CW];
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
        for (int j = 0; j < CW; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // the epilogue's bias values are requested now (round 6: loaded behind the K loop they were one more exposed round trip of a launch
    // whose waves live ~9-15 us)
    float bias_r[CW];
#pragma unroll
    for (int j = 0; j < CW; ++j) bias_r[j] = (kw == 0) ? a.bias[(cb + j) * 32 + c32] : 0.f;
    if (live) {
        // row sources: the second one's pointer is moved back by the first one's channels, so a chunk's address is `pointer + KC q` in both
        const float* p1[RW];
        const float* p2[RW];
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const int rr = min((ru * RW + i) * 32 + c32, a.R - 1);
            const int s1 = a.g1 ? (a.g1m ? (rr / a.g1m) * a.g1n : 0) + a.g1[rr] : rr;
            p1[i] = a.x1 + (size_t)s1 * a.ld1 + (KC / 2) * hl;
            p2[i] = p1[i];
            if (a.c2) {
                const int s2 = a.g2 ? (a.g2m ? (rr / a.g2m) * a.g2n : 0) + a.g2[rr] : rr;
                p2[i] = a.x2 + (size_t)s2 * a.ld2 + (KC / 2) * hl - (size_t)KC * nq1;
            }
        }
        const wvec* wq = static_cast<const wvec*>(a.wp) + (size_t)cb * nq * WV * 64 + lane;
        const size_t wstride = (size_t)nq * WV * 64;  // vectors between consecutive column blocks
        // A ring of PD K chunks in flight: a wave's loop is a chain of dependent round trips to L2 / MALL (the weights of a layer are read
        // once per 32-row block), and one chunk in flight left the launch latency-bound; the ring is refilled in place behind its last
        // reader.  Round 6: the `#pragma unroll 8` loop that the fp32 form had before was NOT unrolled ("-Wpass-failed: loop not unrolled",
        // then silenced by the Makefile's -Wno-pass-failed): every 8-wide K chunk was a load, a wait for it and four MFMAs -- one exposed L2
        // round trip per chunk, eight to sixteen of them per ~9 us launch.
        constexpr int PD = Op::template pd<RW, CW>();
        float4 xr[PD][RW][XV];
        wvec wr[PD][CW][WV];
        auto fetch = [&](int slot, int q) __attribute__((always_inline)) {
            q = min(q, qb - 1);  // (past the end: a harmless repeat of the last chunk, never used)
#pragma unroll
            for (int i = 0; i < RW; ++i) {
                const float* s = (q < nq1 ? p1[i] : p2[i]) + KC * q;
#pragma unroll
                for (int v = 0; v < XV; ++v) xr[slot][i][v] = *reinterpret_cast<const float4*>(s + 4 * v);
            }
#pragma unroll
            for (int j = 0; j < CW; ++j)
#pragma unroll
                for (int v = 0; v < WV; ++v) wr[slot][j][v] = wq[(size_t)j * wstride + ((size_t)q * WV + v) * 64];
        };
        auto products = [&](int slot) __attribute__((always_inline)) { Op::template products<RW, CW>(xr[slot], wr[slot], acc); };
#pragma unroll
        for (int d = 0; d < PD; ++d) fetch(d, qa + d);
        int q0 = qa;
        // full groups of PD chunks whose refills all exist: straight-line code (a branch inside the group made the compiler drain every
        // load at each join).  Round 6: the loop stops one group early -- it used to refill past the end of the slice (a clamped repeat of
        // the last chunk: 2-4 wasted chunk requests of the 8-24 a wave makes)
#pragma unroll 1
        for (; q0 + 2 * PD <= qb; q0 += PD) {
#pragma unroll
            for (int d = 0; d < PD; ++d) {
                products(d);
                // the refill goes into the registers the products just read (issued earlier it needs other registers and a drained copy at
                // the loop's end), in program order: the wait in front of slot d + 1 leaves the PD - 1 younger refills in flight
                __builtin_amdgcn_sched_barrier(0);
                fetch(d, q0 + d + PD);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // the ring holds the next PD chunks; fewer than 2 PD are left.  Slices whose length is a multiple of PD (every layer of the network)
        // need no further request; the others fetch their last few chunks behind the products that free the slot
#pragma unroll
        for (int d = 0; d < PD; ++d) {
            if (q0 + d < qb) {
                products(d);
                if (q0 + d + PD < qb) fetch(d, q0 + d + PD);
            }
        }
#pragma unroll
        for (int d = 0; d < PD - 1; ++d)
            if (q0 + PD + d < qb) products(d);
    }
    if constexpr (SK > 1) {
        // partial blocks of the K slices 1 .. SK-1 go through LDS (register-major: conflict-free), slice 0 adds them up in slice order
        if (kw > 0) {
            float* dst = red + ((size_t)(ruw * (SK - 1) + (kw - 1)) * RW * CW * 16) * 64 + lane;
#pragma unroll
            for (int i = 0; i < RW; ++i)
#pragma unroll
                for (int j = 0; j < CW; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) dst[((i * CW + j) * 16 + r) * 64] = acc[i][j][r];
        }
        __syncthreads();
        if (kw > 0) return;
#pragma unroll
        for (int s = 0; s < SK - 1; ++s) {
            const float* src = red + ((size_t)(ruw * (SK - 1) + s) * RW * CW * 16) * 64 + lane;
#pragma unroll
            for (int i = 0; i < RW; ++i)
#pragma unroll
                for (int j = 0; j < CW; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] += src[((i * CW + j) * 16 + r) * 64];
        }
    }
    if (!live) return;
    // C layout: register r of lane (hl, c32) = row (r & 3) + 8 * (r >> 2) + 4 * hl, column c32 of the block
#pragma unroll
    for (int j = 0; j < CW; ++j) {
        const int col = (cb + j) * 32 + c32;
        const float bb = bias_r[j];
#pragma unroll
        for (int i = 0; i < RW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (ru * RW + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
                float v = acc[i][j][r] + bb;
                if (a.leaky) v = leaky02(v);
                if (row < a.R) a.y[(size_t)row * a.ldy + col] = v;
            }
    }
}
