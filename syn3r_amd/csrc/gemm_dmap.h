// k_gemm_dmap: the persistent form of the 256 x 160 LDS-DMA kernel.
// Included by gemm.hip inside its anonymous namespace (one translation unit; the kernels share GemmParams, the epilogues and the
// LDS-DMA pieces of gemm_common.h / gemm_dma160.h).

// ---------------------------------------------------------------------------------------------
// PERSISTENT form of the 256-row LDS-DMA kernel (k_gemm_dma<MODE, 256>), used for the temporal convolutions and the dense
// contractions that stay on the 256 x 160 tile (the 3x3 convolutions measured 1-3 % slower with it and keep one tile per block).  Same tile, ring (3 slots of 53,248 B), staggered wavefronts
// and per-lane im2col addressing; what changes is what happens at a tile boundary:
//   - the block walks its XCD's share of the tiles (one block per CU, as k_gemm_widep);
//   - the DMA ISSUE CURSOR runs on across tile boundaries: stages are numbered through the block's whole tile list, the
//     ring slot of stage g is g mod 3, and during the last two k-tiles of a tile the cursor already requests the first
//     two stages of the next one - their L2 / HBM latency hides behind this tile's epilogue;
//   - the epilogue therefore has ONE slot (the last one read) instead of the whole ring: the accumulators go through it
//     in two passes of 32 rows per wavefront (lean_store<2>: 8 x 5,632 B = 45 KB), stores drain under the next k-loop.
// vmcnt bookkeeping: a stage wait is "all but the one younger stage" (vmcnt(6), as k_gemm_dma) except for the first
// k-tile after an epilogue, where the epilogue's loads and stores sit between the two prefetched stages: vmcnt(0)
// (both stages were requested a whole epilogue earlier).
template <int MODE>
__global__ void __launch_bounds__(512, 2) k_gemm_dmap(GemmParams p) {
    constexpr int BM = 256, STAGE = DMA256_STAGE;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wn = wv & 1;
    const int tiles_n = (p.N + BN - 1) / BN;
    const int tiles_m = (p.M + BM - 1) / BM;
    const XcdTiles tiles = xcd_tiles((unsigned)(tiles_m * tiles_n));
    const int nkt = p.K / BK;

    // ---- issue cursor: per-lane source state of the tile whose stages are being requested
    const int cpb = (MODE == MODE_DENSE) ? 1 : p.Cin / BK;
    const int prow = lane >> 3;
    const int csrc = (lane & 7) ^ prow;                 // source 16-byte chunk that lands in slot (lane & 7)
    const int nb = wv < 4 ? 3 : 2;                      // B pieces of this wavefront (20 in total: 3,3,3,3,2,2,2,2)
    const int b_first = wv < 4 ? wv * 3 : 12 + (wv - 4) * 2;
    DmaSrc160<MODE, 3> src;
    unsigned itl = blockIdx.x / 8;                      // the cursor's position in this block's tile list ...
    int ikt = 0, islot = 0;                             // ... k-tile inside that tile, ring slot of the next stage
    // row tile of position `rt` in the tile order (GemmParams::tc_pb: temporal convolutions walk the frames of a pixel block first)
    auto row_tile = [&](unsigned rt) -> int {
        if constexpr (MODE == MODE_TCONV) {
            if (p.tc_pb > 0) { const unsigned pb = rt / (unsigned)p.tc_nf, fr_ = rt - pb * (unsigned)p.tc_nf; return (int)(fr_ * (unsigned)p.tc_pb + pb); }
        }
        return (int)rt;
    };
    auto issue_next = [&]() -> bool {     // request the next stage of the block's stage sequence; false: none left
        if (itl >= tiles.len) return false;
        if (ikt == 0) {
            const unsigned tile = tiles.start + itl;
            src.set_tile(p, wv, prow, csrc, nb, b_first, row_tile(tile / (unsigned)tiles_n) * BM, (int)(tile % (unsigned)tiles_n) * BN);
        }
        src.issue(p, wv, nb, b_first, cpb, smem_raw + islot * STAGE, DMA256_A_BYTES);
        if (++ikt == nkt) { ikt = 0; itl += tiles.stride; }
        if (++islot == 3) islot = 0;
        return true;
    };

    const unsigned lds0 = lds_addr(smem_raw);
    const Frag160 frag(lane, wm, wn, DMA256_A_BYTES);
    const bool defer = wv >= 4;           // stagger of the SIMD partners (see k_gemm_widep)

    int issued = 0, consumed = 0;         // stages requested / stages whose k-tile has been multiplied (wave-uniform)
    if (issue_next()) ++issued;
    if (issue_next()) ++issued;
    int cslot = 0;
    bool first_tile = true;
    for (unsigned tl = blockIdx.x / 8; tl < tiles.len; tl += tiles.stride) {
        const unsigned tile = tiles.start + tl;
        const int m0 = row_tile(tile / (unsigned)tiles_n) * BM, n0 = (int)(tile % (unsigned)tiles_n) * BN;
        float4v acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = (float4v){0.f, 0.f, 0.f, 0.f};
        half8 a0[TM], b0[TN], a1[TM], b1[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) { asm volatile("" : "=v"(a0[i])); asm volatile("" : "=v"(a1[i])); }   // (not live across tiles)
#pragma unroll
        for (int j = 0; j < TN; ++j) { asm volatile("" : "=v"(b0[j])); asm volatile("" : "=v"(b1[j])); }
        for (int kt = 0; kt < nkt; ++kt) {
            // the stage of this k-tile has landed once only the ONE younger stage (6..7 loads of this wavefront) is in flight
            if ((kt == 0 && !first_tile) || issued - consumed < 2) WAIT_VMCNT(0);
            else WAIT_VMCNT(DMA_PIECES_MIN);
            __builtin_amdgcn_s_barrier();
            if (defer && kt > 0) mma160(acc, a1, b1);    // second k-half of the previous stage (fragments read before the barrier)
            if (issue_next()) ++issued;              // overwrites the slot read one iteration ago (all wavefronts are past it)
            ktile160(lds0 + (unsigned)cslot * STAGE, frag, acc, a0, b0, a1, b1);
            if (!defer) mma160(acc, a1, b1);
            ++consumed;
            if (++cslot == 3) cslot = 0;
        }
        if (defer) mma160(acc, a1, b1);
        first_tile = false;
        __syncthreads();   // every wavefront is done reading the last stage: its slot is the epilogue's staging area
        {
            const int last = cslot == 0 ? 2 : cslot - 1;
            int le = lane;                    // opaque per tile: the epilogue's lane-derived indices stay inside the tile loop
            asm volatile("" : "+v"(le));
            __half* st = (__half*)(smem_raw + last * STAGE) + wv * (32 * EPI_LD);
            const int gm0 = m0 + wm * WM, gn0 = n0 + wn * WN;
            const bool full = gm0 + WM <= p.M && gn0 + WN <= p.N;
            lean_store<2, true>(p, acc, st, le, gm0, gn0, p.N, p.bias, p.residual, p.aux, full);
            lean_store<2, true>(p, acc + 2, st, le, gm0 + 32, gn0, p.N, p.bias, p.residual, p.aux, full);
        }
        // (the next tile's first barrier orders these staging reads before the DMA that reuses the slot)
    }
}

// 16-byte chunk swizzle of LDS images with 64-byte rows (4 chunks): slot = chunk ^ s(row >> 2 & 3) with s = (0,2,3,1) keeps every
// 16-lane group of a ds_read_b128 fragment read on 16 different 16-byte bank units (k_lnlin320's weight stages).
__device__ __forceinline__ int h_swz(int row_in_16) { return (0x78 >> (2 * (row_in_16 >> 2))) & 3; }
