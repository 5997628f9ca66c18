// What the LDS-DMA kernels on the 160-column tile share (k_gemm_dma, k_gemm_dmap, k_gemm_dmapd): the ring geometry, the counted waits,
// the per-lane im2col source of a stage's DMA (DmaSrc160) and the k-tile body (Frag160, ktile160, mma160).
// Included by gemm.hip inside its anonymous namespace, in front of the three kernels.

// ---------------------------------------------------------------------------------------------
// LDS-DMA pipelined variant (default).  global_load_lds (16 B per lane, per-lane source address = an
// im2col gather for the convolutions, a zero page for padding / out-of-range rows) writes straight into a
// 3-stage LDS ring; a counted s_waitcnt vmcnt leaves the next stage's DMA in flight across ONE raw
// s_barrier per k-tile, so two k-tiles (104 KB per CU) of loads are always outstanding and no VGPRs or
// ds_write instructions are spent on staging.  The LDS image is lane-linear per wave-instruction (8 rows x
// 128 B), so the XOR swizzle is applied to the per-lane SOURCE chunk and undone by the fragment reads.
// hipcc would put s_waitcnt vmcnt(0) in front of any ds_read it can see while a DMA is pending, so the
// fragment reads are inline asm (ds_read_b128 + counted lgkmcnt, operands tied through "+v").
__device__ __half g_zero_page[64];   // zero-initialised: source of padded chunks

constexpr int DMA_B_BYTES = BN * BK * 2;                  // 20480
// BM = 256: 512 threads, 3-stage ring (156 KB, one block per CU, two k-tiles of DMA in flight).
// BM = 128: 256 threads, 2-stage ring (72 KB, TWO blocks per CU): a block's prologue DMA latency and its
//           40-80 KB store tail (store-issue bound at ~10 B/clk/CU) are hidden behind the other block's MFMAs
//           instead of idling the CU; costs 1.4x the L2->LDS bytes per output row (B tile per 128 rows).
constexpr int DMA256_A_BYTES = 256 * BK * 2;                       // 32,768
constexpr int DMA256_STAGE = DMA256_A_BYTES + DMA_B_BYTES;         // 53,248
constexpr int DMA256_LDS = 3 * DMA256_STAGE;                       // 159,744 B: the ring of the 256-row kernels

// The counted waits.  A stage is 1 KB pieces (8 rows x 128 B, one global_load_lds per wavefront): every wavefront issues its own
// 32 rows of A (4 pieces) and its share of the 20 B pieces - eight wavefronts 3,3,3,3,2,2,2,2, four wavefronts 5 each.  "All but the
// one younger stage have landed" is therefore vmcnt(fewest pieces a wavefront issues per stage): a wavefront that issues one more
// waits for one load of the younger stage too, never for less than its own stage.
constexpr int DMA_A_PIECES = 4, DMA_B_PIECES = BN / 8;             // per wavefront / per stage
constexpr int DMA_PIECES_MIN = DMA_A_PIECES + DMA_B_PIECES / 8;    // 6: BM = 256, wavefronts 4-7
constexpr int DMA_PIECES_128 = DMA_A_PIECES + DMA_B_PIECES / 4;    // 9: BM = 128, every wavefront
constexpr int FRAG_READS = TM + TN;                                // 9 ds_read_b128 per k-half
static_assert(DMA_PIECES_MIN == 6 && DMA_PIECES_128 == 9 && FRAG_READS == 9, "the waits below were counted for these");
#define WAIT_VMCNT(N) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory")

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

#define DS_READ128(dst, addr, OFF) asm volatile("ds_read_b128 %0, %1 offset:" #OFF : "=v"(dst) : "v"(addr))

__device__ __forceinline__ unsigned lds_addr(const char* smem) { return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)smem; }

// ---- per-lane source state of the tile whose stages are being requested (NB_MAX = B pieces per wavefront: 3 = eight wavefronts, 5 = four)
// DMA assignment: lane -> (row within an 8-row piece, destination slot); source chunk un-swizzled.
// Source addresses advance incrementally: stages are issued in k order, a k-tile inside one filter tap is
// +128 bytes on every live row, and the full im2col arithmetic (64-bit multiplies, bounds tests) runs only
// when the tap changes (every Cin/64 k-tiles).  Padded rows point at the zero page and do not advance.
// The per-lane constants (prow, csrc: row within an 8-row piece and source chunk; nb, b_first: the wavefront's B pieces; cpb:
// k-tiles per filter tap) stay locals of the kernel and come in as arguments: as members of this struct they share its fate in
// the optimiser (kept in memory until the unrolled loops index the arrays with constants) and k_gemm_dmap came out with 1-3 more
// scalar spills per instantiation.
template <int MODE, int NB_MAX>
struct DmaSrc160 {
    const __half* a_base[4];
    int a_n[4], a_y[4], a_x[4];
    const __half* a_cur[4];
    int a_inc[4];                         // halfs per k-tile: BK for live rows, 0 for zero-page rows
    const __half* b_cur[NB_MAX];
    int b_inc[NB_MAX];
    int tap_next = 0, c_left = 0;         // wave-uniform: next tap to set up, k-tiles left in the current tap

    // row decomposition of the tile at (m0, n0).  a2 (dense, wave-uniform): the rows come from the second source p.A2
    __device__ __forceinline__ void set_tile(const GemmParams& p, int wv, int prow, int csrc, int nb, int b_first, int m0, int n0, bool a2 = false) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + wv * 32 + i * 8 + prow;
            const int mc = m < p.M ? m : p.M - 1;
            if constexpr (MODE == MODE_DENSE) {
                // A-tiled: rows past M exist in the padded last row block (never stored); the k advance is one tile image
                const int last_rb = (p.M + 127) >> 7, rb = (m >> 7) < last_rb ? (m >> 7) : last_rb - 1;
                a_base[i] = p.a_tiled ? p.A + (long long)rb * (p.K >> 6) * 8192 + (m & 127) * 64 + csrc * 8
                                      : p.A + (long long)mc * p.lda + csrc * 8;
                if (a2) a_base[i] = p.A2 + (long long)mc * p.lda2 + csrc * 8;
                a_n[i] = a_y[i] = a_x[i] = 0;
                a_cur[i] = a_base[i]; a_inc[i] = p.a_tiled ? 8192 : BK;
            } else if constexpr (MODE == MODE_CONV2D) {
                const int hw = p.Ho * p.Wo;
                a_n[i] = mc / hw;
                const int r = mc - a_n[i] * hw;
                a_y[i] = r / p.Wo;
                a_x[i] = r - a_y[i] * p.Wo;
                a_base[i] = p.A + csrc * 8;
            } else {
                a_y[i] = (mc / p.HW) % p.F;
                a_n[i] = a_x[i] = 0;
                a_base[i] = p.A + (long long)mc * p.Cin + csrc * 8;
            }
        }
#pragma unroll
        for (int j = 0; j < NB_MAX; ++j) {
            const int n = n0 + (b_first + j) * 8 + prow;
            const bool ok = j < nb && n < p.N;
            b_cur[j] = ok ? p.W + (long long)n * p.K + csrc * 8 : g_zero_page;
            b_inc[j] = ok ? BK : 0;
        }
        tap_next = 0; c_left = 0;
    }
    __device__ __forceinline__ void set_tap(const GemmParams& p, int tap) {
        if constexpr (MODE == MODE_CONV2D) {
            const int dy = tap / 3 - p.pad, dx = tap % 3 - p.pad;
            const int Hg = p.ups ? p.Hi * 2 : p.Hi, Wg = p.ups ? p.Wi * 2 : p.Wi;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int yy = a_y[i] * p.stride + dy, xx = a_x[i] * p.stride + dx;
                const bool ok = yy >= 0 && yy < Hg && xx >= 0 && xx < Wg;
                if (p.ups) { yy >>= 1; xx >>= 1; }
                const long long off = (((long long)a_n[i] * p.Hi + yy) * p.Wi + xx) * p.Cin;
                a_cur[i] = ok ? a_base[i] + off : g_zero_page;
                a_inc[i] = ok ? BK : 0;
            }
        } else if constexpr (MODE == MODE_TCONV) {
            const int df = tap - 1;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ff = a_y[i] + df;
                const bool ok = ff >= 0 && ff < p.F;
                a_cur[i] = ok ? a_base[i] + (long long)df * p.HW * p.Cin : g_zero_page;
                a_inc[i] = ok ? BK : 0;
            }
        }
    }
    // request the tile's next stage into the ring slot at `st` (A image of a_bytes, then B).  Stages must be issued in k order
    __device__ __forceinline__ void issue(const GemmParams& p, int wv, int nb, int b_first, int cpb, char* st, int a_bytes) {
        if constexpr (MODE != MODE_DENSE) {
            if (c_left == 0) { set_tap(p, tap_next); ++tap_next; c_left = cpb; }
            --c_left;
        }
#pragma unroll
        for (int i = 0; i < DMA_A_PIECES; ++i) {
            __builtin_amdgcn_global_load_lds((gbl_void_t*)a_cur[i], (lds_void_t*)(st + (wv * 4 + i) * 1024), 16, 0, 0);
            a_cur[i] += a_inc[i];
        }
#pragma unroll
        for (int j = 0; j < NB_MAX; ++j) {
            if (j < nb) {
                __builtin_amdgcn_global_load_lds((gbl_void_t*)b_cur[j], (lds_void_t*)(st + a_bytes + (b_first + j) * 1024), 16, 0, 0);
                b_cur[j] += b_inc[j];
            }
        }
    }
};

// ---- fragment addressing (byte offsets inside a stage whose A image is a_bytes long)
struct Frag160 {
    unsigned a_row, b_row, sw0, sw1;
    __device__ __forceinline__ Frag160(int lane, int wm, int wn, int a_bytes) {
        const int fr = lane & 15, fq = lane >> 4;
        a_row = (unsigned)((wm * WM + fr) * 128);
        b_row = (unsigned)(a_bytes + (wn * WN + fr) * 128);
        sw0 = (unsigned)(((0 + fq) ^ (fr & 7)) << 4); sw1 = (unsigned)(((4 + fq) ^ (fr & 7)) << 4);
    }
};

// one k-half's 4 x 5 MFMA group
__device__ __forceinline__ void mma160(float4v (&acc)[TM][TN], const half8 (&a)[TM], const half8 (&b)[TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[j], a[i], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);    // (behind the first group: keeps the second wait behind it)
}

// One k-tile of the stage at LDS address sb: the fragment reads of both k-halves, the first half's MFMAs as soon as its
// FRAG_READS reads have landed (the second half's FRAG_READS still in flight), then the wait for the second half, whose MFMAs
// (mma160(acc, a1, b1)) the caller places: at once, or behind the next barrier for the staggered wavefronts.
__device__ __forceinline__ void ktile160(unsigned sb, const Frag160& f, float4v (&acc)[TM][TN], half8 (&a0)[TM], half8 (&b0)[TN],
                                         half8 (&a1)[TM], half8 (&b1)[TN]) {
    {
        const unsigned aa = sb + f.a_row + f.sw0, ba = sb + f.b_row + f.sw0;
        DS_READ128(a0[0], aa, 0); DS_READ128(a0[1], aa, 2048); DS_READ128(a0[2], aa, 4096); DS_READ128(a0[3], aa, 6144);
        DS_READ128(b0[0], ba, 0); DS_READ128(b0[1], ba, 2048); DS_READ128(b0[2], ba, 4096); DS_READ128(b0[3], ba, 6144);
        DS_READ128(b0[4], ba, 8192);
    }
    {
        const unsigned aa = sb + f.a_row + f.sw1, ba = sb + f.b_row + f.sw1;
        DS_READ128(a1[0], aa, 0); DS_READ128(a1[1], aa, 2048); DS_READ128(a1[2], aa, 4096); DS_READ128(a1[3], aa, 6144);
        DS_READ128(b1[0], ba, 0); DS_READ128(b1[1], ba, 2048); DS_READ128(b1[2], ba, 4096); DS_READ128(b1[3], ba, 6144);
        DS_READ128(b1[4], ba, 8192);
    }
    static_assert(TM == 4 && TN == 5, "the reads above and the operand lists below are written out for 4 + 5 fragments");
    asm volatile("s_waitcnt lgkmcnt(%[younger])"
                 : "+v"(a0[0]), "+v"(a0[1]), "+v"(a0[2]), "+v"(a0[3]), "+v"(b0[0]), "+v"(b0[1]), "+v"(b0[2]), "+v"(b0[3]), "+v"(b0[4])
                 : [younger] "i"(FRAG_READS));
    mma160(acc, a0, b0);
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a1[0]), "+v"(a1[1]), "+v"(a1[2]), "+v"(a1[3]), "+v"(b1[0]), "+v"(b1[1]), "+v"(b1[2]), "+v"(b1[3]), "+v"(b1[4]));
}
