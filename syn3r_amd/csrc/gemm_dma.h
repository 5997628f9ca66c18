// k_gemm_dma (BM x 160 tile on an LDS-DMA ring, one tile per block; EPI: its epilogue) and k_splitk_finish.
// Included by gemm.hip inside its anonymous namespace (one translation unit; the kernels share GemmParams, the epilogues and the
// LDS-DMA pieces of gemm_common.h / gemm_dma160.h, where the ring and its counted waits are described).

// EPI: which epilogue the tile leaves through - a compile-time choice, so that the general one carries no branch for the others.
// The split-activation epilogues (gemm_common.h) serve the LPIPS "fp16x2" mode: MODE_CONV2D, BM = 256, never with split-K.
enum { EPI_GENERAL = 0, EPI_SPLIT_OUT = 1, EPI_SPLIT_MASK = 2 };      // gemm_epilogue / split_epilogue<true> / split_epilogue<false>

template <int MODE, int BM, int EPI = EPI_GENERAL>
__global__ void __launch_bounds__(BM * 2, 2) k_gemm_dma(GemmParams p) {
    constexpr int DMA_STAGES = BM == 256 ? 3 : 2;
    constexpr int NWAVES = BM / 32;                          // 8 or 4
    constexpr int DMA_A_BYTES = BM * BK * 2;
    constexpr int DMA_STAGE_BYTES = DMA_A_BYTES + DMA_B_BYTES;
    constexpr int NB_MAX = (20 + NWAVES - 1) / NWAVES;       // B pieces per wavefront: 3 (8 waves) or 5 (4 waves)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wn = wv & 1;
    const int tiles_n = (p.N + BN - 1) / BN;
    const int tiles_m = (p.M + BM - 1) / BM;
    const unsigned ntile = (unsigned)(tiles_m * tiles_n);
    // split-K: which part of the K range.  An XCD takes ONE K part (blocks b and b + 8 share an XCD: part = (b % 8) % S) and a
    // contiguous chunk of that part's tiles, so that it streams 1 / S of the weight panel and 1 / (8 / S) of the rows instead of the
    // whole panel (round 4's order gave every XCD both parts of its tiles: counted HBM bytes 4.1x the algorithmic ones on the
    // M = 4 032 launches, profiles/r04/traffic.json).  Speed only: any placement computes the same partial tiles.
    int sp = 0;
    unsigned bid;
    if (p.ksplit > 1 && (ntile * (unsigned)p.ksplit) % 8 == 0 && 8 % p.ksplit == 0) {
        const unsigned xcd = blockIdx.x % 8, k = blockIdx.x / 8, S = (unsigned)p.ksplit;
        sp = (int)(xcd % S);
        bid = (xcd / S) * (ntile * S / 8) + k;
    } else {
        sp = p.ksplit > 1 ? (int)(blockIdx.x / ntile) : 0;
        bid = xcd_remap(blockIdx.x - (unsigned)sp * ntile, ntile);
    }
    const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int nkt = p.ksplit > 1 ? p.K / BK / p.ksplit : p.K / BK;
    const int kt0 = sp * nkt;            // split-K: this block's part starts at k-tile kt0, possibly inside a filter tap
    const int prow = lane >> 3;
    const int csrc = (lane & 7) ^ prow;                 // source 16-byte chunk that lands in slot (lane & 7)
    // B pieces issued by this wavefront (20 in total): 8 waves -> 3,3,3,3,2,2,2,2 ; 4 waves -> 5 each
    const int nb = NWAVES == 8 ? (wv < 4 ? 3 : 2) : 5;
    const int b_first = NWAVES == 8 ? (wv < 4 ? wv * 3 : 12 + (wv - 4) * 2) : wv * 5;
    const int cpb = (MODE == MODE_DENSE) ? 1 : p.Cin / BK;
    DmaSrc160<MODE, NB_MAX> src;
    // two sources (split-K launches only, parts never straddle K1): the parts from k-tile K1 / BK on read A2
    src.set_tile(p, wv, prow, csrc, nb, b_first, m0, n0, MODE == MODE_DENSE && p.A2 && p.ksplit > 1 && kt0 >= p.K1 / BK);
    if (p.ksplit > 1) {
#pragma unroll
        for (int j = 0; j < NB_MAX; ++j) src.b_cur[j] += (long long)kt0 * src.b_inc[j];
        if constexpr (MODE == MODE_DENSE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) src.a_cur[i] += (long long)(kt0 - ((p.A2 && kt0 >= p.K1 / BK) ? p.K1 / BK : 0)) * src.a_inc[i];
        } else {
            const int rem = kt0 % cpb;   // k-tiles of the tap already behind this part
            src.tap_next = kt0 / cpb;
            src.set_tap(p, src.tap_next);
            ++src.tap_next;
            src.c_left = cpb - rem;
#pragma unroll
            for (int i = 0; i < 4; ++i) src.a_cur[i] += (long long)rem * src.a_inc[i];
        }
    }
    auto issue_stage = [&](int buf) { src.issue(p, wv, nb, b_first, cpb, smem_raw + buf * DMA_STAGE_BYTES, DMA_A_BYTES); };     // stages in k order
    issue_stage(0);
    if (nkt > 1) issue_stage(1);

    float4v acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (float4v){0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15, fq = lane >> 4;
    const unsigned lds0 = lds_addr(smem_raw);
    const Frag160 frag(lane, wm, wn, DMA_A_BYTES);

    // BM = 256 (two wavefronts per SIMD behind one barrier): wavefronts 4-7 defer every stage's second MFMA group past
    // the next barrier (stagger: DESIGN.md section 4, round 2): they multiply while their SIMD partners issue DMA and read fragments.
    half8 a0[TM], b0[TN], a1[TM], b1[TN];
    const bool defer = (BM == 256) && wv >= 4;
    int buf = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        if constexpr (DMA_STAGES == 3) {
            // stage kt has landed once at most one later stage (6..7 loads of this wavefront) is still in flight
            if (kt + 1 < nkt) WAIT_VMCNT(DMA_PIECES_MIN);
            else WAIT_VMCNT(0);
        } else {
            // two slots: only in the first iteration is a younger stage (9 loads) already in flight
            if (kt == 0 && nkt > 1) WAIT_VMCNT(DMA_PIECES_128);
            else WAIT_VMCNT(0);
        }
        __builtin_amdgcn_s_barrier();
        if (defer && kt > 0) mma160(acc, a1, b1);    // second k-half of stage kt-1 (fragments read before the barrier)
        if constexpr (DMA_STAGES == 3) {
            if (kt + 2 < nkt) {
                int nbuf = buf + 2; if (nbuf >= DMA_STAGES) nbuf -= DMA_STAGES;
                issue_stage(nbuf);              // stage kt + 2 overwrites the stage read in iteration kt-1 (all waves are past it)
            }
        } else {
            if (kt >= 1 && kt + 1 < nkt) issue_stage(buf ^ 1);           // stage kt + 1 into the slot read in iteration kt-1
        }
        ktile160(lds0 + (unsigned)buf * DMA_STAGE_BYTES, frag, acc, a0, b0, a1, b1);
        if (!defer) mma160(acc, a1, b1);
        if (++buf == DMA_STAGES) buf = 0;
    }
    if (defer) mma160(acc, a1, b1);
    if (p.ksplit > 1) {                  // fp32 partial tile of this K part: acc[i][j] = rows i*16 + fr, four columns j*16 + fq*4 ..
        float* ws = p.split_ws + (size_t)sp * p.M * p.N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm * WM + i * 16 + fr;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WN + j * 16 + fq * 4;
                if (m < p.M && n < p.N) *(float4v*)(ws + (size_t)m * p.N + n) = acc[i][j];      // (N % 8 == 0: whole quads)
            }
        }
        return;
    }
    __syncthreads();   // every wavefront is done reading the ring before the epilogue reuses it
    if constexpr (EPI == EPI_GENERAL) gemm_epilogue(p, acc, smem_raw, lane, wv, wm, wn, m0, n0, tile_n);
    else split_epilogue<EPI == EPI_SPLIT_OUT>(p, acc, smem_raw, lane, wv, wm, wn, m0, n0);
}

// The second half of a split-K contraction: out = epilogue(sum over the K parts, in order) with gemm_epilogue's arithmetic
// (bias and row vector added in fp32, scaled, rounded to fp16; then the residual / aux blend on the rounded value).
// One thread per 8 output columns.
__global__ void __launch_bounds__(256) k_splitk_finish(GemmParams p) {
    const int nch = p.N / 8;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)p.M * nch) return;
    const int m = (int)(q / nch), n = (int)(q - (long long)m * nch) * 8;
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = 0.f;
    for (int s = 0; s < p.ksplit; ++s) {
        const float4v* src = (const float4v*)(p.split_ws + ((size_t)s * p.M + m) * p.N + n);
        const float4v a = src[0], b = src[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) { f[e] += a[e]; f[4 + e] += b[e]; }
    }
    if (p.bias) {
        const half8 b = *(const half8*)(p.bias + n);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] += (float)b[e];
    }
    if (p.rowvec) {
        const half8 t = *(const half8*)(p.rowvec + (long long)rowvec_index(m, p.rows_per_vec, p.rv_group) * p.ldrv + n);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] += (float)t[e];
    }
    half8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (_Float16)(f[e] * p.s_acc);
    if (p.residual || p.aux) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (float)v[e];
        if (p.residual) {
            const half8 r = *(const half8*)(p.residual + (long long)m * p.ldr + n);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] += p.s_res * (float)r[e];
        }
        if (p.aux) {
            const half8 a = *(const half8*)(p.aux + (long long)m * p.ldaux + n);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] += p.s_aux * (float)a[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (_Float16)f[e];
    }
    *(half8*)(p.out + (long long)m * p.ldc + n) = v;
}
