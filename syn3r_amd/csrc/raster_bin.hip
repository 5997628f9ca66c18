// Gaussian rasteriser, tile binning: from the projected Gaussians (k_preprocess, raster_fwd.hip) to the per-tile lists the blend
// kernels walk.  Two paths: the hierarchical filter ("Hierarchical binning" below) and, for images of more than kMaxSuper
// super-tiles, the pair sort (sort.hip).  The rest of the rasteriser sees raster_bin_prepare / raster_bin_lists (raster_common.h).
#include "common.h"
#include "raster_common.h"

using namespace syn3r;

namespace syn3r {

size_t binning_bytes(long long P) {
    size_t n = (size_t)(P > 0 ? P : 1);
    return 2 * align256(n * 8) + 2 * align256(n * 4) + sort_scratch_bytes(n) + 256;
}

BinningState carve_binning(void* buf, long long P) {
    size_t n = (size_t)(P > 0 ? P : 1);
    char* p = (char*)buf;
    BinningState b;
    b.keys_a = (unsigned long long*)p; p += align256(n * 8);
    b.keys_b = (unsigned long long*)p; p += align256(n * 8);
    b.vals_a = (unsigned*)p; p += align256(n * 4);
    b.vals_b = (unsigned*)p; p += align256(n * 4);
    b.sort_scratch = p;
    return b;
}

}  // namespace syn3r

namespace {

// (tile id, Gaussian id) pairs, emitted in DEPTH order (position i of `order`), wave-cooperatively: the 64
// Gaussians of a wavefront own one contiguous output range; lane l of every 64-pair slice finds its owner by a
// 6-step search over the wavefront's exclusive tile counts (kept in registers, read by cross-lane shuffles) and
// writes one pair -> fully coalesced stores and no per-lane loops over differently sized tile rectangles.
__global__ void __launch_bounds__(256) k_dup_tiles(int N, const unsigned* __restrict__ order,
                                                   const float* __restrict__ means2D, const int* __restrict__ radii,
                                                   const unsigned* __restrict__ offsets, int gx, int gy,
                                                   unsigned* __restrict__ keys, unsigned* __restrict__ vals,
                                                   unsigned cap, unsigned* __restrict__ header,
                                                   uint2* __restrict__ ranges, int tiles) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    for (int t = i; t < tiles; t += gridDim.x * 256) ranges[t] = make_uint2(0u, 0u);   // k_tile_ranges fills the non-empty ones
    const int lane = threadIdx.x & 63;
    const bool valid = i < N;
    unsigned id = valid ? order[i] : 0u;
    int r = valid ? radii[id] : 0;
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    if (r > 0) tile_rect(means2D[2 * (size_t)id], means2D[2 * (size_t)id + 1], r, gx, gy, x0, y0, x1, y1);
    const int w = x1 - x0;
    const unsigned cnt = (unsigned)(w * (y1 - y0));
    // wave-exclusive prefix of the counts; the output range starts at the first lane's global offset
    const unsigned incl = wave_scan_incl(cnt);
    const unsigned local = incl - cnt;
    const unsigned total = __shfl(incl, 63, 64);
    const int first = blockIdx.x * 256 + (threadIdx.x & ~63);       // < N for every launched wavefront with work
    const unsigned base = first < N ? offsets[first] : 0u;
    const float inv_w = w > 0 ? 1.0f / (float)w : 0.0f;
    for (unsigned t = 0; t < total; t += 64) {
        const unsigned p = t + lane;
        int j = 0;
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {                   // largest j with local_j <= p
            unsigned lc = __shfl(local, j + step, 64);
            if (lc <= p) j += step;
        }
        const unsigned k = p - __shfl(local, j, 64);
        const int xj = __shfl(x0, j, 64), yj = __shfl(y0, j, 64), wj = __shfl(w, j, 64);
        const float iwj = __shfl(inv_w, j, 64);
        const unsigned idj = __shfl(id, j, 64);
        if (p < total) {
            // k / wj for k < 2^21: (k + 0.5) / wj is never within rounding distance of an integer
            const int ty = (int)(((float)k + 0.5f) * iwj);
            int tyc = ty;
            if ((unsigned)(tyc * wj) > k) --tyc;                      // reciprocal-multiply guard (at most one off)
            else if ((unsigned)((tyc + 1) * wj) <= k) ++tyc;
            const int tx = (int)k - tyc * wj;
            const unsigned o = base + p;
            if (o < cap) {
                keys[o] = (unsigned)((yj + tyc) * gx + xj + tx);
                vals[o] = idj;
            } else {
                header[1] = 1u;   // capacity overflow (asynchronous mode only): the caller re-renders
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_tile_ranges(long long P_cap, const unsigned* __restrict__ header,
                                                     const unsigned* __restrict__ keys,
                                                     uint2* __restrict__ ranges) {
    long long P = (long long)header[0];
    if (P > P_cap) P = P_cap;
    long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    unsigned cur = keys[i];
    if (i == 0) ranges[cur].x = 0;
    else {
        unsigned prev = keys[i - 1];
        if (cur != prev) {
            ranges[prev].y = (unsigned)i;
            ranges[cur].x = (unsigned)i;
        }
    }
    if (i == P - 1) ranges[cur].y = (unsigned)P;
}

// ---------------------------------------------------------------------------------------------
// Hierarchical binning (round 5): the per-tile lists WITHOUT a pair sort and WITHOUT a global depth sort.
// The published pipeline duplicates every Gaussian into (tile, depth) keys and sorts them; rounds 1-4 of this build argsorted the
// Gaussians by depth (4 passes, 12 launches of 49 blocks: launch latency), emitted the pairs in that order and stably sorted them by
// tile id (two 7-bit passes over 2.6 M pairs) - 260 of the 950 us of a 1080p iteration.  A tile's list is the set of Gaussians whose
// tile rectangle holds the tile, ordered by (depth bits, index); so the lists are built by filtering and ordered where they are short:
//   super-tiles of 4 x 4 tiles (510 at 1080p; 8 x 8 where that would be more than 512: up to ~4K);
//   k_super_count / k_super_append  the Gaussians in chunks (index order): per (chunk, super-tile) the number of Gaussians whose
//                                   rectangle meets the super-tile (one LDS atomic each); every append block sums the count table's
//                                   columns itself (no scan launch) and appends its (depth bits << 32 | index) keys to the
//                                   super-tiles' lists, unordered inside the chunk;
//   k_super_sort                    a block per super-tile sorts its list (1 015 keys on average, 3 201 at most at 200 000 Gaussians)
//                                   in LDS - a bitonic network on 8-byte keys; longer lists are sorted in LDS-sized pieces and merged
//                                   through global memory - and leaves, in order, the ids and the rectangles clipped to the
//                                   super-tile (4 x 4 bits); its wavefronts then count, per tile of the super-tile, the entries
//                                   whose rectangle holds the tile (round 6: until then a launch of its own, a block per tile);
//   k_tile_offsets / k_tile_write   one single-block scan over the tiles (ranges, pair count, overflow flag, the blend kernels' tile
//                                   order), then a block per tile (four wavefronts, a quarter of the super-tile's list each,
//                                   coalesced, 2 B per entry) writes the entries whose rectangle holds the tile.
// Same lists as the (tile << 32 | depth) key sort, entry for entry - equal depths in index order, as a stable sort leaves them
// (tests/test_raster_gpu.py, test_raster_full_gpu.py against the oracle's sort); five launches where there were twenty-seven.
// Shapes it does not take (more than 512 super-tiles: images beyond ~4K) keep the argsort and the pair sort.
constexpr int kBinThreads = 512;          // Gaussians per round of a binning block
constexpr int kOffThreads = 1024;         // k_tile_offsets: one block
#ifndef SYN3R_MAX_SUPER
#define SYN3R_MAX_SUPER 512
#endif
constexpr int kMaxSuper = SYN3R_MAX_SUPER;     // (developer builds: -DSYN3R_MAX_SUPER=2048 takes 1080p to 2 x 2-tile super-tiles, profiles/r06/binning_supertiles.txt)

// Super-tiles of the SMALLEST side (1, 2, 4, 8 tiles) that gives at most 512 of them: 4 x 4 at 1080p (510 super-tiles, a block per
// list sorts ~1 000 keys), 8 x 8 up to ~4K; 2 x 2 at the LLFF / DTU image sizes the reference trains on (504 x 378: 192 super-tiles -
// with 4 x 4 its 48 lists of a 200 000-Gaussian model were ~4x longer than the LDS piece and k_super_sort's single-block global-
// memory merge took 370 of the iteration's 957 us, profiles/r06/raster_breakdown_504x378.txt), single tiles below 512
// tiles; `ss` = log2 of the side.  The Gaussians go through the count / append kernels in chunks of
// rounds x 512, as many chunks as keep the (chunk, super-tile) count table within kBinCounters.
struct BinPlan { int ss, sgx, sgy, nsuper, rounds, nchunks; bool ok; };
inline BinPlan bin_plan(int N, int gx, int gy) {
    BinPlan b;
    for (b.ss = 0; b.ss <= 3; ++b.ss) {
        const int side = 1 << b.ss;
        b.sgx = (gx + side - 1) / side; b.sgy = (gy + side - 1) / side;
        b.nsuper = b.sgx * b.sgy;
        if (b.nsuper <= kMaxSuper) break;
    }
    if (b.ss > 3) b.ss = 3;
    b.ok = b.nsuper <= kMaxSuper;
    const int max_chunks = b.ok ? (int)(kBinCounters / (size_t)b.nsuper) : 1;
    const int units = (N + kBinThreads - 1) / kBinThreads;
    b.rounds = (units + max_chunks - 1) / max_chunks;
    if (b.rounds < 1) b.rounds = 1;
    b.nchunks = (units + b.rounds - 1) / b.rounds;
    return b;
}

// does this shape take the hierarchical binning?  (SYN3R_BIN_HIER=0 in tuning builds: the pair sort, for A/B runs)
inline bool hier_binning(int N, int gx, int gy) {
    static const int on = tune_env("SYN3R_BIN_HIER", 1);
    return on != 0 && bin_plan(N, gx, gy).ok;
}

// the tile rectangle of Gaussian i (empty for culled ones)
struct BinRect { int x0, y0, x1, y1; };
__device__ __forceinline__ BinRect bin_rect(int i, int N, const float* __restrict__ means2D, const int* __restrict__ radii, int gx, int gy) {
    BinRect r; r.x0 = r.y0 = r.x1 = r.y1 = 0;
    if (i < N) {
        const int rad = radii[i];
        if (rad > 0) tile_rect(means2D[2 * (size_t)i], means2D[2 * (size_t)i + 1], rad, gx, gy, r.x0, r.y0, r.x1, r.y1);
    }
    return r;
}
__device__ __forceinline__ unsigned short clip_rect(const BinRect& q, int sx, int sy, int ss) {   // x0 | x1 << 4 | y0 << 8 | y1 << 12, each 0..8
    const int bx = sx << ss, by = sy << ss, side = 1 << ss;
    const int rx0 = max(q.x0 - bx, 0), rx1 = min(q.x1 - bx, side), ry0 = max(q.y0 - by, 0), ry1 = min(q.y1 - by, side);
    return (unsigned short)(rx0 | (rx1 << 4) | (ry0 << 8) | (ry1 << 12));
}

__global__ void __launch_bounds__(kBinThreads) k_super_count(int N, const float* __restrict__ means2D, const int* __restrict__ radii,
                                                             int gx, int gy, int ss, int sgx, int nsuper, int rounds, int nchunks,
                                                             unsigned* __restrict__ counters, unsigned* __restrict__ header) {
    __shared__ unsigned tot[kMaxSuper];
    for (int s = threadIdx.x; s < nsuper; s += kBinThreads) tot[s] = 0u;
    __syncthreads();
    int pairs = 0;            // the EXACT number of (Gaussian, tile) pairs of this block's Gaussians: header[3] (see k_tile_offsets)
    for (int r = 0; r < rounds; ++r) {
        const int i = (blockIdx.x * rounds + r) * kBinThreads + threadIdx.x;
        const BinRect q = bin_rect(i, N, means2D, radii, gx, gy);
        if (q.x1 > q.x0 && q.y1 > q.y0) {
            pairs += (q.x1 - q.x0) * (q.y1 - q.y0);
            const int side1 = (1 << ss) - 1, sx0 = q.x0 >> ss, sx1 = (q.x1 + side1) >> ss, sy0 = q.y0 >> ss, sy1 = (q.y1 + side1) >> ss;
            for (int sy = sy0; sy < sy1; ++sy)
                for (int sx = sx0; sx < sx1; ++sx) atomicAdd(&tot[sy * sgx + sx], 1u);
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < nsuper; s += kBinThreads) counters[(size_t)blockIdx.x * nsuper + s] = tot[s];   // chunk-major: k_super_append reads it coalesced
    // ONE global atomic per block (integer: any order gives the same sum): the wavefronts meet in LDS first - eight atomics per block
    // on one address cost the kernel 8 of its 14 us
    __shared__ unsigned pairs_s;
    if (threadIdx.x == 0) pairs_s = 0u;
    __syncthreads();
    pairs = wave_sum_i(pairs);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(&pairs_s, (unsigned)pairs);
    __syncthreads();
    if (threadIdx.x == 0 && pairs_s) atomicAdd(&header[3], pairs_s);
}

// Appends the keys (depth bits << 32 | index) of this chunk's Gaussians to the lists of the super-tiles their rectangles meet.
// Where the chunk's entries of a super-tile start: the (chunk, super-tile) counts are not scanned by a launch of their own - every
// block sums the table's columns (a few parts per super-tile, coalesced over the super-tiles; a few hundred KB of L2 reads per
// block), a wavefront scans the totals, block 0 publishes the list starts for the kernels that follow.
__global__ void __launch_bounds__(kBinThreads) k_super_append(int N, const float* __restrict__ depths, const float* __restrict__ means2D,
                                                              const int* __restrict__ radii, int gx, int gy, int ss, int sgx, int nsuper,
                                                              int rounds, int nchunks, const unsigned* __restrict__ counters,
                                                              unsigned* __restrict__ sstart, unsigned cap,
                                                              unsigned long long* __restrict__ skeys, unsigned* __restrict__ header) {
    __shared__ unsigned run[kMaxSuper];            // next free position of (super-tile, this chunk)
    __shared__ unsigned tot_s[kMaxSuper], pre_s[kMaxSuper];
    __shared__ unsigned part_tot[kMaxSuper > kBinThreads ? kMaxSuper : kBinThreads], part_pre[kMaxSuper > kBinThreads ? kMaxSuper : kBinThreads];   // nsuper * PARTS <= max(kBinThreads, nsuper)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    {
        const int PARTS = max(1, min(8, kBinThreads / nsuper));  // (super-tile, part) items: one per thread, one pass
        const int per = (nchunks + PARTS - 1) / PARTS;
        for (int w = threadIdx.x; w < nsuper * PARTS; w += kBinThreads) {
            const int s_ = w % nsuper, part = w / nsuper;
            const int c0 = part * per, c1 = min(nchunks, c0 + per);
            unsigned tot = 0, pre = 0;
            constexpr int UN = 32;
            for (int cb = c0; cb < c1; cb += UN) {
                unsigned c[UN];
#pragma unroll
                for (int u = 0; u < UN; ++u) c[u] = cb + u < c1 ? counters[(size_t)(cb + u) * nsuper + s_] : 0u;
#pragma unroll
                for (int u = 0; u < UN; ++u) { tot += c[u]; pre += cb + u < (int)blockIdx.x ? c[u] : 0u; }
            }
            part_tot[w] = tot; part_pre[w] = pre;
        }
        __syncthreads();
        for (int s_ = threadIdx.x; s_ < nsuper; s_ += kBinThreads) {
            unsigned tot = 0, pre = 0;
            for (int k = 0; k < PARTS; ++k) { tot += part_tot[k * nsuper + s_]; pre += part_pre[k * nsuper + s_]; }
            tot_s[s_] = tot; pre_s[s_] = pre;
        }
        __syncthreads();
        if (wv == 0) {
            constexpr int PER = kMaxSuper / 64;
            unsigned c[PER], sum = 0;
#pragma unroll
            for (int k = 0; k < PER; ++k) { const int s_ = lane * PER + k; c[k] = s_ < nsuper ? tot_s[s_] : 0u; sum += c[k]; }
            const unsigned incl = wave_scan_incl(sum);
            unsigned ex = incl - sum;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int s_ = lane * PER + k;
                if (s_ < nsuper) {
                    run[s_] = ex + pre_s[s_];
                    if (blockIdx.x == 0) sstart[s_] = ex;
                }
                ex += c[k];
            }
            if (blockIdx.x == 0 && lane == 63) { sstart[nsuper] = incl; header[2] = incl; }
        }
        __syncthreads();
    }
    for (int r = 0; r < rounds; ++r) {
        const int i = (blockIdx.x * rounds + r) * kBinThreads + threadIdx.x;
        const BinRect q = bin_rect(i, N, means2D, radii, gx, gy);
        if (q.x1 > q.x0 && q.y1 > q.y0) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(depths[i]) << 32) | (unsigned)i;
            const int side1 = (1 << ss) - 1, sx0 = q.x0 >> ss, sx1 = (q.x1 + side1) >> ss, sy0 = q.y0 >> ss, sy1 = (q.y1 + side1) >> ss;
            for (int sy = sy0; sy < sy1; ++sy)
                for (int sx = sx0; sx < sx1; ++sx) {
                    const unsigned o = atomicAdd(&run[sy * sgx + sx], 1u);
                    if (o < cap) skeys[o] = key;
                    else header[1] = 1u;
                }
        }
    }
}

// the list of super-tile s: [sstart[s], sstart[s + 1]) clipped to the capacity
__device__ __forceinline__ void super_range(int s, const unsigned* __restrict__ sstart, unsigned cap, unsigned& b, unsigned& e) {
    b = min(sstart[s], cap); e = min(sstart[s + 1], cap);
}

// A block per super-tile: its list of keys into ascending order (depth bits, then index: what a stable sort by depth leaves), then
// the ids and clipped rectangles of the entries.  Bitonic network in the form whose every comparison puts the smaller key at the
// lower index (first step of a merge: partner l ^ (k - 1); later steps: l + j), so the virtual +inf padding up to a power of two
// never moves and any length sorts.  Up to kSortLds keys (every list of the 200 000-Gaussian benchmark: 3 201 at most) the whole
// network runs in LDS; beyond, LDS-sized pieces are sorted,
// and for the larger merges the steps whose distance reaches across pieces run on global memory (one block: __syncthreads orders
// them), the rest again in LDS.
constexpr int kSortLds = 4096;                    // keys per LDS piece (32 KB: four blocks per CU, every super-tile's block resident at once)
constexpr int kSuperSortThreads = 1024;
__device__ __forceinline__ void cmpx(unsigned long long& a, unsigned long long& b) { if (a > b) { const unsigned long long t = a; a = b; b = t; } }
// pair of comparison t in a step of distance j (a power of two): l = t with a zero inserted at bit log2(j), r = l + j
__device__ __forceinline__ int pair_lo(int t, int j) { return (t << 1) - (t & (j - 1)); }
// The steps of the network on `buf[0, m)` (m a power of two, LDS) are taken TWO per pass: a thread owns the four keys that two
// consecutive steps connect, exchanges them in registers and stores them - half the barriers and half the LDS round trips of a
// step per pass (the network is bound by those, not by its comparisons: 78 steps -> 42 passes at 4 096 keys).
// distances j, j/2, .. 1 of a merge (pairs (l, l + j)), two distances per pass, a last single one if their number is odd
__device__ __forceinline__ void bitonic_dists(unsigned long long* buf, int m, int j) {
    for (; j >= 2; j >>= 2) {
        const int jh = j >> 1;
        for (int t = threadIdx.x; t < (m >> 2); t += kSuperSortThreads) {
            const int e0 = pair_lo(pair_lo(t, jh), j);
            unsigned long long a = buf[e0], b = buf[e0 + jh], c = buf[e0 + j], d = buf[e0 + j + jh];
            cmpx(a, c); cmpx(b, d);          // distance j
            cmpx(a, b); cmpx(c, d);          // distance j / 2
            buf[e0] = a; buf[e0 + jh] = b; buf[e0 + j] = c; buf[e0 + j + jh] = d;
        }
        __syncthreads();
    }
    if (j == 1) {
        for (int t = threadIdx.x; t < (m >> 1); t += kSuperSortThreads) cmpx(buf[2 * t], buf[2 * t + 1]);
        __syncthreads();
    }
}
// all steps of merge size k: the flip step (pairs (l, l ^ (k - 1)) inside blocks of k) together with distance k / 4, then the rest
__device__ __forceinline__ void bitonic_merge(unsigned long long* buf, int m, int k) {
    if (k == 2) {
        for (int t = threadIdx.x; t < (m >> 1); t += kSuperSortThreads) cmpx(buf[2 * t], buf[2 * t + 1]);
        __syncthreads();
        return;
    }
    const int q = k >> 2;
    for (int t = threadIdx.x; t < (m >> 2); t += kSuperSortThreads) {
        const int off = t & (q - 1), blk = (t - off) << 2;           // (t / q) * k
        const int ia = blk + off, ib = ia + q, ird = blk + (k - 1 - off), irc = ird - q;
        unsigned long long a = buf[ia], b = buf[ib], c = buf[irc], d = buf[ird];
        cmpx(a, d); cmpx(b, c);              // flip
        cmpx(a, b); cmpx(c, d);              // distance k / 4
        buf[ia] = a; buf[ib] = b; buf[irc] = c; buf[ird] = d;
    }
    __syncthreads();
    bitonic_dists(buf, m, q >> 1);
}

__device__ __forceinline__ bool rect_has(unsigned r, int rx, int ry) {
    return rx >= (int)(r & 15u) && rx < (int)((r >> 4) & 15u) && ry >= (int)((r >> 8) & 15u) && ry < (int)(r >> 12);
}

constexpr int kBinUnroll = 8;
// k_tile_write: a block per tile, its four wavefronts a quarter of the super-tile's list each (the longest list sets the kernel's
// time: a wavefront per tile left the tiles of the busiest super-tile walking ~8 000 entries while the rest of the chip had finished).
__device__ __forceinline__ void tile_quarter(unsigned b, unsigned e, int q, unsigned& qb, unsigned& qe) {
    const unsigned len = (e - b + 3u) / 4u;
    qb = min(e, b + (unsigned)q * len); qe = min(e, qb + len);
}

// The per-tile, per-quarter entry counts of super-tile (sx, sy) (tcount[4 t + q], what k_tile_offsets scans and k_tile_write starts
// from) by the block that has just ordered the list: wavefront w takes tiles w, w + 16, ... of the super-tile and walks the clipped
// rectangles (2 B per entry: in LDS where the list was sorted there, else as written a moment ago by this block - visible after
// the barrier: one workgroup, one CU), quarter by quarter.  Until round 6 a launch of its own (k_tile_count, a block per tile:
// 10 us + a launch at 1080p).
__device__ __forceinline__ void super_tile_counts(int sx, int sy, int ss, int gx, int gy, unsigned n, const unsigned short* srect_b,
                                                  unsigned* __restrict__ tcount) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, side = 1 << ss;
    const unsigned len = (n + 3u) / 4u;                        // tile_quarter's split of [0, n)
    // (tile, quarter) items over the block's 16 wavefronts: 2 x 2-tile super-tiles (the LLFF sizes, lists of ~10 000) keep all of
    // them busy, 4 x 4 gives a wavefront the four quarters of one tile.  Per-lane counts on the vector unit and one cross-lane sum
    // per item (the scalar unit is shared by the CU's wavefronts: per-chunk ballot masks doubled this kernel's time); four chunks
    // of 64 entries are requested before the first is tested (the long lists are read from global memory).
    for (int it = wv; it < side * side * 4; it += kSuperSortThreads / 64) {
        const int ti = it >> 2, q = it & 3;
        const int rx = ti & (side - 1), ry = ti >> ss;
        const int tx = (sx << ss) + rx, ty = (sy << ss) + ry;
        if (tx >= gx || ty >= gy) continue;                    // (wave-uniform)
        const unsigned lo = min(n, (unsigned)q * len), hi = min(n, lo + len);
        unsigned cnt = 0;
        for (unsigned i0 = lo; i0 < hi; i0 += 256) {
            unsigned short r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = srect_b[min(i0 + u * 64 + lane, hi - 1u)];
#pragma unroll
            for (int u = 0; u < 4; ++u) cnt += (i0 + u * 64 + lane < hi && rect_has(r[u], rx, ry)) ? 1u : 0u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0) tcount[4 * ((size_t)ty * gx + tx) + q] = cnt;
    }
}

// (8 wavefronts per SIMD = two blocks per CU: 510 blocks at 1080p are resident at once - at 72 registers only one block fits and the
// kernel runs its blocks in two rounds, 36 -> 70 us)
__global__ void __launch_bounds__(kSuperSortThreads, 8) k_super_sort(int N, const float* __restrict__ means2D, const int* __restrict__ radii,
                                                                  int gx, int gy, int ss, int sgx, const unsigned* __restrict__ sstart, unsigned cap,
                                                                  unsigned long long* __restrict__ skeys, unsigned* __restrict__ sid,
                                                                  unsigned short* __restrict__ srect, unsigned* __restrict__ tcount) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];   // kSortLds keys
    const int s_ = blockIdx.x, sx = s_ % sgx, sy = s_ / sgx;
    unsigned b, e;
    super_range(s_, sstart, cap, b, e);
    const int n = (int)(e - b);
    if (n == 0) { super_tile_counts(sx, sy, ss, gx, gy, 0u, srect, tcount); return; }     // (zeros for its tiles)
    unsigned long long* gk = skeys + b;
    const unsigned long long INF = ~0ull;
    int m = 1;
    while (m < n) m <<= 1;
    const unsigned long long* sorted;              // where the sorted keys end up
    if (m <= kSortLds) {
        for (int i = threadIdx.x; i < m; i += kSuperSortThreads) sk[i] = i < n ? gk[i] : INF;
        __syncthreads();
        for (int k = 2; k <= m; k <<= 1) bitonic_merge(sk, m, k);
        sorted = sk;
    } else {
        // pieces of kSortLds keys, each through the whole network in LDS
        for (int p0 = 0; p0 < n; p0 += kSortLds) {
            for (int i = threadIdx.x; i < kSortLds; i += kSuperSortThreads) sk[i] = p0 + i < n ? gk[p0 + i] : INF;
            __syncthreads();
            for (int k = 2; k <= kSortLds; k <<= 1) bitonic_merge(sk, kSortLds, k);
            for (int i = threadIdx.x; i < kSortLds; i += kSuperSortThreads) if (p0 + i < n) gk[p0 + i] = sk[i];
            __syncthreads();
        }
        // merges across pieces: the steps of distance >= kSortLds on global memory (a partner beyond n is +inf: nothing to do)
        for (int k = kSortLds << 1; k <= m; k <<= 1) {
            const int h = k >> 1;
            for (int t = threadIdx.x; t < (m >> 1); t += kSuperSortThreads) {
                const int off = t & (h - 1), l = pair_lo(t, h), r = l - off + (k - 1 - off);
                if (r < n) { unsigned long long a = gk[l], c = gk[r]; if (a > c) { gk[l] = c; gk[r] = a; } }
            }
            __syncthreads();
            for (int j = k >> 2; j >= kSortLds; j >>= 1) {
                for (int t = threadIdx.x; t < (m >> 1); t += kSuperSortThreads) {
                    const int l = pair_lo(t, j), r = l + j;
                    if (r < n) { unsigned long long a = gk[l], c = gk[r]; if (a > c) { gk[l] = c; gk[r] = a; } }
                }
                __syncthreads();
            }
            for (int p0 = 0; p0 < n; p0 += kSortLds) {            // distances below a piece: in LDS
                for (int i = threadIdx.x; i < kSortLds; i += kSuperSortThreads) sk[i] = p0 + i < n ? gk[p0 + i] : INF;
                __syncthreads();
                bitonic_dists(sk, kSortLds, kSortLds >> 1);
                for (int i = threadIdx.x; i < kSortLds; i += kSuperSortThreads) if (p0 + i < n) gk[p0 + i] = sk[i];
                __syncthreads();
            }
        }
        sorted = gk;
    }
    if (sorted == sk) {
        // (n <= kSortLds = 4 x kSuperSortThreads) the clipped rectangles also go to LDS - over the keys, once every thread has read
        // its ids - where the tile counts read them: 2 B per entry and tile from global memory, one dependent load per 64 entries,
        // made the longest list's block the kernel's time (36 -> 74 us)
        unsigned short clip[kSortLds / kSuperSortThreads];
#pragma unroll
        for (int u = 0; u < kSortLds / kSuperSortThreads; ++u) {
            const int i = threadIdx.x + u * kSuperSortThreads;
            clip[u] = 0;
            if (i < n) {
                const unsigned id = (unsigned)sk[i];
                const BinRect q = bin_rect((int)id, N, means2D, radii, gx, gy);
                clip[u] = clip_rect(q, sx, sy, ss);
                sid[b + i] = id;
                srect[b + i] = clip[u];
            }
        }
        __syncthreads();
        unsigned short* sr = (unsigned short*)sk;
#pragma unroll
        for (int u = 0; u < kSortLds / kSuperSortThreads; ++u) {
            const int i = threadIdx.x + u * kSuperSortThreads;
            if (i < n) sr[i] = clip[u];
        }
        __syncthreads();
        super_tile_counts(sx, sy, ss, gx, gy, (unsigned)n, sr, tcount);
        return;
    }
    for (int i = threadIdx.x; i < n; i += kSuperSortThreads) {
        const unsigned id = (unsigned)sorted[i];
        const BinRect q = bin_rect((int)id, N, means2D, radii, gx, gy);
        sid[b + i] = id;
        srect[b + i] = clip_rect(q, sx, sy, ss);
    }
    __syncthreads();                 // the block's rectangles are in memory for the block
    super_tile_counts(sx, sy, ss, gx, gy, (unsigned)n, srect + b, tcount);
}

// ranges[t] = (start, end) of tile t's list, clipped to the capacity; header[0] = the pair count, header[1] = 1 if it (or the
// super-tile lists) did not fit.  One block, any tile count.
__global__ void __launch_bounds__(kOffThreads) k_tile_offsets(int tiles, const unsigned* __restrict__ tcount, unsigned cap,
                                                              uint2* __restrict__ ranges, unsigned* __restrict__ header,
                                                              unsigned* __restrict__ tile_order) {
    __shared__ unsigned smem[kOffThreads / 64 + 1];
    __shared__ unsigned bh[256];
    if (tile_order) { for (int k = threadIdx.x; k < 256; k += kOffThreads) bh[k] = 0u; __syncthreads(); }
    constexpr int PER = 8;                                       // consecutive tiles per thread: 8 192 tiles per round
    unsigned carry = 0;
    for (int start = 0; start < tiles; start += kOffThreads * PER) {
        const int t0 = start + threadIdx.x * PER;
        unsigned c[PER], sum = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            c[k] = 0u;
            if (t0 + k < tiles) { const uint4 q4 = ((const uint4*)tcount)[t0 + k]; c[k] = (q4.x + q4.y) + (q4.z + q4.w); }
            sum += c[k];
        }
        unsigned total;
        unsigned ex = block_exclusive_scan<kOffThreads / 64>(sum, smem, total) + carry;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            // an empty tile is (0, 0), as k_tile_ranges leaves it
            if (t0 + k < tiles) ranges[t0 + k] = c[k] ? make_uint2(min(ex, cap), min(ex + c[k], cap)) : make_uint2(0u, 0u);
            if (tile_order && t0 + k < tiles) atomicAdd(&bh[255u - min(255u, c[k] >> 5)], 1u);
            ex += c[k];
        }
        carry += total;
    }
    if (tile_order) {        // tiles by descending list length (buckets of 32 entries): the blend kernels take the long ones first
        __syncthreads();
        if (threadIdx.x < 64) {                                   // exclusive scan of the 256 bucket counts: 4 per lane
            const int l = threadIdx.x;
            unsigned c[4], sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { c[k] = bh[4 * l + k]; sum += c[k]; }
            unsigned ex = wave_scan_incl(sum) - sum;
#pragma unroll
            for (int k = 0; k < 4; ++k) { bh[4 * l + k] = ex; ex += c[k]; }
        }
        __syncthreads();
        for (int t = threadIdx.x; t < tiles; t += kOffThreads) {
            const uint4 q4 = ((const uint4*)tcount)[t];
            const unsigned c = (q4.x + q4.y) + (q4.z + q4.w);
            tile_order[atomicAdd(&bh[255u - min(255u, c >> 5)], 1u)] = (unsigned)t;
        }
    }
    if (threadIdx.x == 0) {
        // `carry` sums the per-tile counts taken from super-tile lists that are CLIPPED to the capacity: once a render overflows it
        // under-counts (every key past `cap` is dropped and uncounted), and a caller that sizes its next buffer from header[0] would
        // at best double per round.  header[3] is the exact pair count (sum of the tile rectangles' areas, k_super_count): reported
        // whenever the lists did not fit, so ONE re-render recovers (tests/test_raster_gpu.py).
        const bool over = carry > cap || header[2] > cap;
        header[0] = over ? max(carry, max(header[3], header[2])) : carry;
        if (over) header[1] = 1u;
    }
}

__global__ void __launch_bounds__(256) k_tile_write(int gx, int tiles, int ss, int sgx, const unsigned* __restrict__ sstart, unsigned cap,
                                                    const unsigned* __restrict__ sid, const unsigned short* __restrict__ srect,
                                                    const uint2* __restrict__ ranges, const unsigned* __restrict__ tcount,
                                                    unsigned* __restrict__ point_list) {
    const int t = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tx = t % gx, ty = t / gx;
    unsigned b, e;
    super_range((ty >> ss) * sgx + (tx >> ss), sstart, cap, b, e);
    tile_quarter(b, e, q, b, e);
    const int rx = tx & ((1 << ss) - 1), ry = ty & ((1 << ss) - 1);
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint4 q4 = ((const uint4*)tcount)[t];
    unsigned pos = ranges[t].x + (q > 0 ? q4.x : 0u) + (q > 1 ? q4.y : 0u) + (q > 2 ? q4.z : 0u);
    for (unsigned i0 = b; i0 < e; i0 += 64 * kBinUnroll) {       // wave-uniform trip count
        unsigned short r[kBinUnroll];
        unsigned id[kBinUnroll];
#pragma unroll
        for (int u = 0; u < kBinUnroll; ++u) {
            const unsigned i = i0 + u * 64 + lane;
            r[u] = i < e ? srect[i] : (unsigned short)0;
            id[u] = i < e ? sid[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kBinUnroll; ++u) {
            const bool hit = rect_has(r[u], rx, ry);
            const unsigned long long m = __ballot(hit);
            if (hit) {
                const unsigned o = pos + (unsigned)__popcll(m & lt);
                if (o < cap) point_list[o] = id[u];
            }
            pos += (unsigned)__popcll(m);
        }
    }
}

int bits_for(unsigned v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

}  // namespace

namespace syn3r {

bool raster_tiles_ordered(int N, int gx, int gy) {
    static const int order_env = tune_env("SYN3R_TILE_ORDER", 1);
    return order_env != 0 && hier_binning(N, gx, gy);
}

int raster_bin_prepare(const GeomState& g, int N, int gx, int gy, bool want_count, hipStream_t stream) {
    if (!hier_binning(N, gx, gy)) {
        // the pair sort: Gaussians by ascending depth (stable: equal depths keep index order), then the tile counts scanned in that
        // order: pairs emitted along it and stably sorted by tile id are ordered like the published (tile << 32 | depth bits) keys
        int in_b = 0;
        int rc = argsort_depth_u32(g.dkeys_a, g.order_a, g.dkeys_b, g.order_b, (size_t)N, g.sort_scratch, stream, &in_b);
        if (rc) return rc;
        if ((in_b ? g.order_b : g.order_a) != g.order) { set_error("raster_preprocess: unexpected argsort parity"); return SYN3R_E_INVALID; }
        return exclusive_scan_u32(g.tiles_touched, g.point_offsets, (size_t)N, g.header, g.scan_scratch, stream, g.order);
    }
    // The hierarchical binning orders and counts on its own (k_super_sort, k_tile_offsets); a caller who asks for the exact pair
    // count before sizing the binning buffer gets the sum of the tile counts
    if (want_count) return exclusive_scan_u32(g.tiles_touched, g.point_offsets, (size_t)N, g.header, g.scan_scratch, stream);
    return SYN3R_OK;
}

int raster_bin_lists(const GeomState& g, const ImageState& im, const BinningState& bn, const int* radii, int N, int gx, int gy,
                     long long P, hipStream_t stream, unsigned** point_list_out, const unsigned** tile_order_out) {
    const size_t tiles = (size_t)gx * gy;
    unsigned* point_list = bn.vals_a;
    unsigned* tile_order = nullptr;
    if (P == 0) {
        if (int rc = check_hip(hipMemsetAsync(im.ranges, 0, tiles * 8, stream), "memset ranges")) return rc;
    } else if (hier_binning(N, gx, gy)) {
        SYN3R_REQUIRE(P < (1ll << 30), "raster_render: pair capacity %lld: the super-tile sort indexes a list with 31-bit integers (2^30 pairs at most)", P);
        const BinPlan bp = bin_plan(N, gx, gy);
        unsigned* counters = im.bin_counters;
        unsigned* sid = bn.vals_b;
        unsigned short* srect = (unsigned short*)bn.keys_a;
        unsigned* sstart = counters + kBinCounters;              // [nsuper + 1] list starts
        unsigned long long* skeys = bn.keys_b;
        static DevOnce once;
        if (int rc = set_max_lds(once, (const void*)k_super_sort, kSortLds * 8, "hipFuncSetAttribute(super_sort)")) return rc;
        SYN3R_LAUNCH(k_super_count, dim3(bp.nchunks), dim3(kBinThreads), 0, stream, N, (const float*)g.means2D, radii, gx, gy, bp.ss, bp.sgx,
                     bp.nsuper, bp.rounds, bp.nchunks, counters, g.header);
        SYN3R_LAUNCH(k_super_append, dim3(bp.nchunks), dim3(kBinThreads), 0, stream, N, (const float*)g.depths, (const float*)g.means2D, radii,
                     gx, gy, bp.ss, bp.sgx, bp.nsuper, bp.rounds, bp.nchunks, (const unsigned*)counters, sstart, (unsigned)P, skeys, g.header);
        SYN3R_LAUNCH(k_super_sort, dim3(bp.nsuper), dim3(kSuperSortThreads), kSortLds * 8, stream, N, (const float*)g.means2D, radii, gx, gy,
                     bp.ss, bp.sgx, (const unsigned*)sstart, (unsigned)P, skeys, sid, srect, im.tile_counts);
        // the blend kernels take the tiles longest list first: with one block per tile in image order they ended on the few long
        // tiles of the last dispatch round (k_render 170 -> 130 us, k_render_bwd 463 -> 380 us at 200 000 Gaussians / 1080p;
        // SYN3R_TILE_ORDER=0 in tuning builds restores the image order)
        if (raster_tiles_ordered(N, gx, gy)) tile_order = im.tile_order;
        SYN3R_LAUNCH(k_tile_offsets, dim3(1), dim3(kOffThreads), 0, stream, (int)tiles, (const unsigned*)im.tile_counts, (unsigned)P,
                     im.ranges, g.header, tile_order);
        SYN3R_LAUNCH(k_tile_write, dim3((unsigned)tiles), dim3(256), 0, stream, gx, (int)tiles, bp.ss, bp.sgx,
                     (const unsigned*)sstart, (unsigned)P, (const unsigned*)sid, (const unsigned short*)srect,
                     (const uint2*)im.ranges, (const unsigned*)im.tile_counts, point_list);
    } else {
        // P is the pair CAPACITY of the binning buffer; the live count is read from the geometry header on
        // the device, so the caller may pass an estimate and skip the device->host read of the exact count
        unsigned* tk_a = (unsigned*)bn.keys_a;
        unsigned* tk_b = (unsigned*)bn.keys_b;
        SYN3R_LAUNCH(k_dup_tiles, dim3(ceil_div(N, 256)), dim3(256), 0, stream, N, g.order, g.means2D, radii,
                           g.point_offsets, gx, gy, tk_a, bn.vals_a, (unsigned)P, g.header, im.ranges, (int)tiles);
        int in_b = 0;
        int rc = sort_pairs_by_tile_u32(tk_a, bn.vals_a, tk_b, bn.vals_b, (size_t)P, bits_for((unsigned)tiles - 1),
                                        bn.sort_scratch, stream, &in_b, g.header);
        if (rc) return rc;
        const unsigned* keys = in_b ? tk_b : tk_a;
        point_list = in_b ? bn.vals_b : bn.vals_a;
        SYN3R_LAUNCH(k_tile_ranges, dim3(ceil_div(P, 256)), dim3(256), 0, stream, P, g.header, keys, im.ranges);
    }
    *point_list_out = point_list;
    *tile_order_out = tile_order;
    return SYN3R_OK;
}

}  // namespace syn3r
