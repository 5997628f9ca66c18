// Mean squared distance of every point to its 3 nearest neighbours.
//
// The reference initialises the Gaussian scales from this quantity inside FSGS' GaussianModel.create_from_pcd
// (`distCUDA2` of the `simple-knn` CUDA extension; reached from gsTrainer construction and from
// reset_gaussians_from_pcd, call site model/diffusionGS.py:1685-1687).  The extension is NOT in /root/reference
// (un-vendored submodule): what it returns is well defined - for point i the mean of the three smallest squared
// Euclidean distances to OTHER points of the cloud - and any exact search returns the same three distances, so this
// file restates the published approach (points ordered along a Morton curve, boxes of consecutive points pruned by
// their bounding boxes) and is checked against brute force (bit-exact, same fp32 operation order) and a k-d tree.
//
// gfx950 mapping: a lane owns one point, lanes of a wavefront hold 64 CONSECUTIVE points of the Morton order, so
// they agree on which boxes survive the pruning test (one ballot per box, no divergent scans) and the scanned
// points are wave-uniform addresses (one 16-byte request per point for the whole wavefront, served by the scalar /
// L1 path).  Work: N * (boxes tested + 1024 * boxes scanned); with a Morton-local cloud 2-10 boxes survive.
// Compiled with -ffp-contract=off (syn3r_amd/build.py STRICT_FP): d2 = (dx*dx + dy*dy) + dz*dz, no fused multiply-add.
#include "common.h"
#include "raster_common.h"

using namespace syn3r;

namespace {

constexpr int kBox = 1024;           // consecutive Morton-ordered points per bounding box
constexpr int kThreads = 256;

// The search exists in two precisions (fp32: the two 3-NN entries; float64: the outlier filter).  Per scalar type: the point
// vector of the Morton-ordered cloud, what rides in its w lane, the "nothing yet" distance, and the names the tracer reports.
template <typename T> struct Scalar;
template <> struct Scalar<float> {
    typedef float4 Vec;
    static constexpr float far = 3.0e38f;
    static constexpr const char *aabb = "k_aabb", *aabb_final = "k_aabb_final", *morton = "k_morton", *gather = "k_gather_idx";
    // the point's original index rides in the w lane (bits, never arithmetic): k_knn3_graph reads it, k_knn3 does not
    static __device__ __forceinline__ float w_lane(unsigned s) { return __uint_as_float(s); }
    static __device__ __forceinline__ float wmin(float v) { return wave_min(v); }
    static __device__ __forceinline__ float wmax(float v) { return wave_max(v); }
};
template <> struct Scalar<double> {
    typedef double4 Vec;
    static constexpr double far = 1.0e300;
    static constexpr const char *aabb = "k_aabb64", *aabb_final = "k_aabb64_final", *morton = "k_morton64", *gather = "k_gather64";
    static __device__ __forceinline__ double w_lane(unsigned) { return 0.0; }
    static __device__ __forceinline__ double wmin(double v) { return wave_min_d(v); }
    static __device__ __forceinline__ double wmax(double v) { return wave_max_d(v); }
};

template <typename T> struct Bounds { T lo[3], hi[3]; };

// Block-reduction tail of both bounding-box levels, in a fixed order: wave shuffles, the four wave results in LDS, thread 0
// combines them and writes out[at].
template <typename T>
__device__ __forceinline__ void block_bounds(T (&lo)[3], T (&hi)[3], Bounds<T>* __restrict__ out, unsigned at) {
    __shared__ T s[kThreads / 64][6];
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = Scalar<T>::wmin(lo[c]); hi[c] = Scalar<T>::wmax(hi[c]); }
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 3; ++c) { s[threadIdx.x >> 6][c] = lo[c]; s[threadIdx.x >> 6][3 + c] = hi[c]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        Bounds<T> b;
        for (int c = 0; c < 3; ++c) {
            b.lo[c] = fmin(fmin(s[0][c], s[1][c]), fmin(s[2][c], s[3][c]));
            b.hi[c] = fmax(fmax(s[0][3 + c], s[1][3 + c]), fmax(s[2][3 + c], s[3][3 + c]));
        }
        out[at] = b;
    }
}

// AABB of points [first, first + count) with stride `per` points per block: out[blockIdx.x]
template <typename T>
__global__ void __launch_bounds__(kThreads) k_aabb(const T* __restrict__ pts, int stride, int n, int per, Bounds<T>* __restrict__ out) {
    const int first = blockIdx.x * per, last = min(n, first + per);
    T lo[3] = {Scalar<T>::far, Scalar<T>::far, Scalar<T>::far}, hi[3] = {-Scalar<T>::far, -Scalar<T>::far, -Scalar<T>::far};
    for (int i = first + threadIdx.x; i < last; i += kThreads) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T v = pts[(size_t)i * stride + c];
            lo[c] = fmin(lo[c], v); hi[c] = fmax(hi[c], v);
        }
    }
    block_bounds(lo, hi, out, blockIdx.x);
}

// one block: AABB of the per-block AABBs
template <typename T>
__global__ void __launch_bounds__(kThreads) k_aabb_final(const Bounds<T>* __restrict__ part, int nparts, Bounds<T>* __restrict__ out) {
    T lo[3] = {Scalar<T>::far, Scalar<T>::far, Scalar<T>::far}, hi[3] = {-Scalar<T>::far, -Scalar<T>::far, -Scalar<T>::far};
    for (int i = threadIdx.x; i < nparts; i += kThreads)
        for (int c = 0; c < 3; ++c) { lo[c] = fmin(lo[c], part[i].lo[c]); hi[c] = fmax(hi[c], part[i].hi[c]); }
    block_bounds(lo, hi, out, 0);
}

__device__ __forceinline__ unsigned spread10(unsigned v) {     // 10 bits -> every third bit
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 30-bit Morton code of the point's cell in a 1024^3 grid over the cloud's bounding box (the ORDER only steers the
// pruning; the distances found do not depend on it)
template <typename T>
__global__ void __launch_bounds__(kThreads) k_morton(const T* __restrict__ pts, int n, const Bounds<T>* __restrict__ bb,
                                                    unsigned* __restrict__ codes) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    unsigned q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const T ext = bb->hi[c] - bb->lo[c];
        T t = ext > T(0) ? (pts[(size_t)i * 3 + c] - bb->lo[c]) / ext : T(0);
        t = fmin(fmax(t * T(1023), T(0)), T(1023));
        q[c] = (unsigned)t;
    }
    codes[i] = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) k_gather(const T* __restrict__ pts, const unsigned* __restrict__ order, int n,
                                                    typename Scalar<T>::Vec* __restrict__ sorted) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned s = order[i];
    sorted[i] = typename Scalar<T>::Vec(pts[(size_t)s * 3], pts[(size_t)s * 3 + 1], pts[(size_t)s * 3 + 2], Scalar<T>::w_lane(s));
}

template <typename V>
__device__ __forceinline__ auto dist2(const V& p, const V& q) {
    const auto dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;                 // the k-d tree's accumulation order for 3 dimensions
}

template <typename T>
__device__ __forceinline__ T box_dist2(const Bounds<T>& b, const typename Scalar<T>::Vec& p) {
    const T dx = fmax(fmax(b.lo[0] - p.x, p.x - b.hi[0]), T(0));
    const T dy = fmax(fmax(b.lo[1] - p.y, p.y - b.hi[1]), T(0));
    const T dz = fmax(fmax(b.lo[2] - p.z, p.z - b.hi[2]), T(0));
    return (dx * dx + dy * dy) + dz * dz;
}

// The box-visiting skeleton of every search here.  A lane owns point p of box `own` and keeps its K best candidates in a state
// the skeleton does not see: scan(b) offers it every point of box b, worst() is its current K-th best squared distance.
// Boxes are visited by a whole wavefront together: its 64 points are consecutive on the curve and inside ONE box (64 divides
// 1024), so `own` is wave-uniform.  The own box comes first: after it the K-th best distance is tight and most other boxes
// fail the test.  Another box is scanned if ANY live lane still needs it - lanes that do not only spend comparisons that
// change nothing.
// Exactness: a box whose nearest face is farther than the current K-th best cannot change the result.  The test is `<=` and
// carries a slack, so it keeps every box that the rounded arithmetic could place just inside, and every box that could hold
// a point exactly as distant as the K-th best (which a caller ordering ties by index may still prefer).
template <typename T, typename Scan, typename Worst>
__device__ __forceinline__ void visit_boxes(const Bounds<T>* __restrict__ boxes, int nboxes, int own, const typename Scalar<T>::Vec& p,
                                            bool live, T slack, Scan scan, Worst worst) {
    const int own_u = __builtin_amdgcn_readfirstlane(own);
    scan(own_u);
    for (int b = 0; b < nboxes; ++b) {
        if (b == own_u) continue;
        const T bd = box_dist2(boxes[b], p);
        const T kth = worst();                             // read outside the `&&`: `live` masks the test, it guards no load
        const bool need = live && bd <= kth * slack;
        if (__ballot(need) == 0ull) continue;
        scan(b);
    }
}

__device__ __forceinline__ void keep3(float d, float& b0, float& b1, float& b2) {     // b0 <= b1 <= b2
    if (d < b2) {
        if (d < b1) {
            b2 = b1;
            if (d < b0) { b1 = b0; b0 = d; } else b1 = d;
        } else b2 = d;
    }
}

__global__ void __launch_bounds__(kThreads) k_knn3(const float4* __restrict__ sorted, const unsigned* __restrict__ order,
                                                  const Bounds<float>* __restrict__ boxes, int n, int nboxes, float* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < n;
    const float4 p = sorted[live ? i : n - 1];
    float b0 = Scalar<float>::far, b1 = Scalar<float>::far, b2 = Scalar<float>::far;
    auto scan = [&](int b) {
        const int first = b * kBox, last = min(n, first + kBox);
        for (int j = first; j < last; ++j) {
            const float d = dist2(p, sorted[j]);          // wave-uniform address
            if (j != i) keep3(d, b0, b1, b2);             // the point itself is masked by its position
        }
    };
    visit_boxes(boxes, nboxes, (live ? i : n - 1) / kBox, p, live, 1.0001f, scan, [&] { return b2; });
    if (live) out[order[i]] = ((b0 + b1) + b2) / 3.0f;
}

// ----------------------------------------------------------------------------------------------------------------
// FSGS' proximity-guided Gaussian unpooling (Zhu et al., ECCV 2024, section 3.2; FSGS' source is not available - every choice the
// paper leaves open is an argument or is stated here, UNPINNED):
//   graph     point i -> the three OTHER points with the smallest d2 = (dx*dx + dy*dy) + dz*dz (no fused multiply-add), ascending
//             by the pair (d2, original index): the index breaks ties, so the graph is unique whatever order the search visits;
//   score     ((d2_0 + d2_1) + d2_2) / 3, the quantity k_knn3 returns (simple-knn's distCUDA2), bit for bit;
//   source    score_i > score_thresh AND max_c log_scale[i,c] > log_scale_thresh (raw log-scales: no exp at the boundary);
//   emission  for the S sources in ascending index order, neighbours nearest first: row 3 * rank + t gets
//             xyz = (xyz_src + xyz_dst) * 0.5f, log-scales / opacity logit / confidence of the DESTINATION, rotation (1,0,0,0).
//             One new Gaussian per directed edge (a -> b and b -> a both grow one).  SH coefficients are zero: the caller's.
// The search is k_knn3's (visit_boxes: same boxes, same pruning test, wave-uniform scans); a lane keeps three 64-bit keys (d2 bits << 32) | index
// - d2 >= 0, so unsigned order on the bits is numeric order and ONE compare gives the (d2, index) order - inserted without a branch
// (min / max on the keys), so that the triple stays in registers.
typedef unsigned long long u64;

__device__ __forceinline__ u64 kmin(u64 a, u64 b) { return a < b ? a : b; }
__device__ __forceinline__ u64 kmax(u64 a, u64 b) { return a < b ? b : a; }

__device__ __forceinline__ void keep3_key(u64 k, u64& b0, u64& b1, u64& b2) {     // b0 <= b1 <= b2
    b2 = kmin(kmax(k, b1), b2);
    b1 = kmin(kmax(k, b0), b1);
    b0 = kmin(k, b0);
}

__global__ void __launch_bounds__(kThreads) k_knn3_graph(const float4* __restrict__ sorted, const Bounds<float>* __restrict__ boxes, int n,
                                                        int nboxes, float* __restrict__ dist2_out, int* __restrict__ index_out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < n;
    const float4 p = sorted[live ? i : n - 1];
    // "nothing yet": k_knn3's 3.0e38f with the largest index, above every real key.  The point itself gets all-ones distance
    // bits - a mask formed from the LOADED index, so the load does not depend on the comparison and four of them issue together.
    const u64 far = ((u64)__float_as_uint(Scalar<float>::far) << 32) | 0xffffffffull;
    const unsigned self = __float_as_uint(p.w);
    u64 b0 = far, b1 = far, b2 = far;
    auto insert = [&](const float4& q) {
        const unsigned id = __float_as_uint(q.w);
        const unsigned hi = __float_as_uint(dist2(p, q)) | (id == self ? 0xffffffffu : 0u);
        keep3_key(((u64)hi << 32) | (u64)id, b0, b1, b2);
    };
    auto scan = [&](int b) {
        const int first = b * kBox, last = min(n, first + kBox);
        int j = first;
        for (; j + 4 <= last; j += 4) {                    // wave-uniform addresses
            const float4 q0 = sorted[j], q1 = sorted[j + 1], q2 = sorted[j + 2], q3 = sorted[j + 3];
            insert(q0); insert(q1); insert(q2); insert(q3);
        }
        for (; j < last; ++j) insert(sorted[j]);
    };
    // the test sees the distance half of the third key: a box that could hold an equally distant point of smaller index stays
    visit_boxes(boxes, nboxes, (live ? i : n - 1) / kBox, p, live, 1.0001f, scan, [&] { return __uint_as_float((unsigned)(b2 >> 32)); });
    if (live) {
        const size_t o = (size_t)__float_as_uint(p.w) * 3;
        dist2_out[o] = __uint_as_float((unsigned)(b0 >> 32));
        dist2_out[o + 1] = __uint_as_float((unsigned)(b1 >> 32));
        dist2_out[o + 2] = __uint_as_float((unsigned)(b2 >> 32));
        index_out[o] = (int)(unsigned)b0; index_out[o + 1] = (int)(unsigned)b1; index_out[o + 2] = (int)(unsigned)b2;
    }
}

// Selection: flag per Gaussian and the number of sources per block of kThreads consecutive Gaussians
__global__ void __launch_bounds__(kThreads) k_unpool_flag(const float* __restrict__ dist2, const float* __restrict__ log_scales, int n,
                                                         float score_thresh, float log_scale_thresh,
                                                         unsigned char* __restrict__ flags, int* __restrict__ block_counts) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    bool sel = false;
    if (i < n) {
        const float score = ((dist2[(size_t)i * 3] + dist2[(size_t)i * 3 + 1]) + dist2[(size_t)i * 3 + 2]) / 3.0f;
        const float ls = fmaxf(fmaxf(log_scales[(size_t)i * 3], log_scales[(size_t)i * 3 + 1]), log_scales[(size_t)i * 3 + 2]);
        sel = score > score_thresh && ls > log_scale_thresh;
        flags[i] = sel ? 1 : 0;
    }
    __shared__ int s[kThreads / 64];
    const int c = __popcll(__ballot(sel));
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
}

// ONE block: exclusive scan of the block counts in block order (a thread sums a contiguous run, the runs are scanned in thread
// order), total -> *count.  No atomics: the offsets, and with them the order of the new rows, do not depend on scheduling.
__global__ void __launch_bounds__(kThreads) k_unpool_scan(const int* __restrict__ block_counts, int nblocks, int* __restrict__ offsets,
                                                         int* __restrict__ count) {
    __shared__ int s[kThreads];
    const int per = (nblocks + kThreads - 1) / kThreads;
    const int first = min(nblocks, (int)threadIdx.x * per), last = min(nblocks, first + per);
    int sum = 0;
    for (int b = first; b < last; ++b) sum += block_counts[b];
    s[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < kThreads; ++t) { const int v = s[t]; s[t] = run; run += v; }
        *count = run;
    }
    __syncthreads();
    int run = s[threadIdx.x];
    for (int b = first; b < last; ++b) { offsets[b] = run; run += block_counts[b]; }
}

// One lane per Gaussian; a source writes its three rows at 3 * (block offset + rank inside the block).  Rows beyond `capacity` and
// neighbour indices outside the cloud are not written (the host has checked both; this keeps a wrong argument inside the buffers).
__global__ void __launch_bounds__(kThreads) k_unpool_emit(const float* __restrict__ xyz, const float* __restrict__ log_scales,
                                                         const float* __restrict__ opacity, const float* __restrict__ confidence,
                                                         const int* __restrict__ index, int n, const unsigned char* __restrict__ flags,
                                                         const int* __restrict__ offsets, int capacity, float* __restrict__ o_xyz,
                                                         float* __restrict__ o_ls, float* __restrict__ o_op, float* __restrict__ o_rot,
                                                         float* __restrict__ o_conf) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const bool sel = i < n && flags[i] != 0;
    __shared__ int s[kThreads / 64];
    const unsigned long long m = __ballot(sel);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s[wave] = __popcll(m);
    __syncthreads();
    if (!sel) return;
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += s[w];
    const long long row0 = 3ll * ((long long)offsets[blockIdx.x] + rank);
    const float sx = xyz[(size_t)i * 3], sy = xyz[(size_t)i * 3 + 1], sz = xyz[(size_t)i * 3 + 2];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const long long r = row0 + t;
        const int d = index[(size_t)i * 3 + t];
        if (r >= capacity || (unsigned)d >= (unsigned)n) continue;
        o_xyz[r * 3] = (sx + xyz[(size_t)d * 3]) * 0.5f;
        o_xyz[r * 3 + 1] = (sy + xyz[(size_t)d * 3 + 1]) * 0.5f;
        o_xyz[r * 3 + 2] = (sz + xyz[(size_t)d * 3 + 2]) * 0.5f;
        o_ls[r * 3] = log_scales[(size_t)d * 3]; o_ls[r * 3 + 1] = log_scales[(size_t)d * 3 + 1]; o_ls[r * 3 + 2] = log_scales[(size_t)d * 3 + 2];
        o_op[r] = opacity[d];
        o_conf[r] = confidence[d];
        *(float4*)(o_rot + r * 4) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    }
}

// ----------------------------------------------------------------------------------------------------------------
// Statistical outlier removal of a point cloud: what the reference runs on the dust3r cloud,
// `down_pcd.remove_statistical_outlier(nb_neighbors=20, std_ratio=3.0)` (model/diffusionGS.py:321, open3d 0.17.0 - not in
// /root/reference).  Published algorithm (Open3D `PointCloud::RemoveStatisticalOutliers`), restated:
//   avg_i  = mean of the Euclidean distances to the nb_neighbors nearest points of the cloud, THE POINT ITSELF INCLUDED
//            (its k-d tree query returns the query point at distance 0), summed nearest first, in float64;
//   mean, std (n - 1 in the denominator) of avg over the cloud;   keep_i = 0 < avg_i < mean + std_ratio * std.
// The same search (prepare<double>, visit_boxes<double>: Morton order, 1024-point boxes, wave-uniform scans), in float64 throughout:
// open3d holds its points as doubles, and the keep decision thresholds a float64 statistic.  A lane keeps its K best
// squared distances sorted in registers (K = 20: 40 VGPRs).
template <int K>
__global__ void __launch_bounds__(kThreads) k_knn_mean64(const double4* __restrict__ sorted, const unsigned* __restrict__ order,
                                                        const Bounds<double>* __restrict__ boxes, int n, int nboxes,
                                                        double* __restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < n;
    const double4 p = sorted[live ? i : n - 1];
    double best[K];                                        // ascending
#pragma unroll
    for (int t = 0; t < K; ++t) best[t] = Scalar<double>::far;
    auto scan = [&](int b) {
        const int first = b * kBox, last = min(n, first + kBox);
        for (int j = first; j < last; ++j) {
            const double d = dist2(p, sorted[j]);          // wave-uniform address; the point itself is a candidate (d = 0)
            if (d < best[K - 1]) {
#pragma unroll
                for (int t = K - 1; t > 0; --t) best[t] = d < best[t - 1] ? best[t - 1] : fmin(best[t], d);
                best[0] = fmin(best[0], d);
            }
        }
    };
    visit_boxes(boxes, nboxes, (live ? i : n - 1) / kBox, p, live, 1.000001, scan, [&] { return best[K - 1]; });
    if (live) {
        const int cnt = n < K ? n : K;                     // a cloud smaller than K: the mean runs over what the query returns
        double sum = 0.0;
#pragma unroll
        for (int t = 0; t < K; ++t)
            if (t < cnt) sum += sqrt(best[t]);
        out[order[i]] = sum / (double)cnt;
    }
}

// ONE block: mean and standard deviation as open3d's PointCloud::RemoveStatisticalOutliers takes them, threshold = mean +
// ratio * std.  The SUMS run over the positive entries only, the DIVISORS are `valid_distances` = the number of points whose
// neighbour query returned anything - every point here (a query returns at least the point itself) - and that count - 1:
// a cluster of more than nb_neighbors coincident points (average distance 0) lowers the mean instead of dropping out of it.
// Thread-strided partial sums + a fixed tree: the result does not depend on scheduling.  stats = {mean, std, threshold, n}
__global__ void __launch_bounds__(1024) k_outlier_stats(const double* __restrict__ avg, int n, double ratio, double* __restrict__ stats) {
    __shared__ double red[1024];
    __shared__ double mean_s;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double v = avg[i];
        if (v > 0.0) s += v;
    }
    auto reduce = [&](double v) {
        red[threadIdx.x] = v;
        __syncthreads();
        for (int o = 512; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        const double r = red[0];
        __syncthreads();
        return r;
    };
    const double total = reduce(s);
    const double valid = (double)n;
    if (threadIdx.x == 0) mean_s = total / valid;
    __syncthreads();
    const double mean = mean_s;
    double q = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const double v = avg[i];
        if (v > 0.0) q += (v - mean) * (v - mean);
    }
    const double sq = reduce(q);
    if (threadIdx.x == 0) {
        const double sd = sqrt(sq / (valid - 1.0));
        stats[0] = mean; stats[1] = sd; stats[2] = mean + ratio * sd; stats[3] = valid;
    }
}

__global__ void __launch_bounds__(kThreads) k_outlier_keep(const double* __restrict__ avg, int n, const double* __restrict__ stats,
                                                          unsigned char* __restrict__ keep) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const double v = avg[i];
    keep[i] = (v > 0.0 && v < stats[2]) ? 1 : 0;
}

// workspace check of every entry: short -> `short_code` (SYN3R_E_WORKSPACE from the graph / unpooling entries, as the header
// documents; SYN3R_E_INVALID from the two older search entries), misaligned -> SYN3R_E_INVALID
int ws_check(const char* who, const void* ws, size_t have, size_t need, int short_code) {
    if (have < need) {
        set_error("%s: workspace too small (%zu < %zu)", who, have, need);
        return short_code;
    }
    SYN3R_REQUIRE(((uintptr_t)ws & 255) == 0, "%s: workspace must be 256-byte aligned", who);
    return SYN3R_OK;
}

// The search workspace, stated once as byte offsets: the *_workspace_bytes entries return `bytes`, prepare() carves by the rest.
template <typename T> struct Layout {
    size_t codes_a, codes_b, order_a, order_b, sorted, part, boxes, sort_ws, bytes;
    explicit Layout(size_t nn) {
        const size_t nbox = (nn + kBox - 1) / kBox;
        size_t at = 0;
        auto take = [&](size_t b) { const size_t o = at; at += align256(b); return o; };
        codes_a = take(nn * 4); codes_b = take(nn * 4);          // Morton codes / order, ping and pong
        order_a = take(nn * 4); order_b = take(nn * 4);
        sorted = take(nn * sizeof(typename Scalar<T>::Vec));     // points in Morton order
        part = take((nbox + 1) * sizeof(Bounds<T>));             // per-box bounds (input order, then sorted order) + the cloud's
        boxes = take((nbox + 1) * sizeof(Bounds<T>));
        sort_ws = at;
        bytes = at + sort_scratch_bytes(nn) + 256;
    }
};

template <typename T> struct Prepared {
    const typename Scalar<T>::Vec* sorted;      // the cloud in Morton order
    const unsigned* order;                      // sorted[i] is points[order[i]]
    const Bounds<T>* boxes;                     // bounds of every kBox consecutive sorted points
    int nbox, blocks;
};

// What every search entry does before its own kernel: check and carve the workspace, then order the cloud.
template <typename T>
int prepare(const char* who, const T* points, int n, void* ws, size_t ws_bytes, int short_code, hipStream_t stream, Prepared<T>* out) {
    const size_t nn = (size_t)n;
    const Layout<T> at(nn);
    if (int rc = ws_check(who, ws, ws_bytes, at.bytes, short_code)) return rc;
    typedef typename Scalar<T>::Vec Vec;
    char* w = (char*)ws;
    unsigned *codes_a = (unsigned*)(w + at.codes_a), *codes_b = (unsigned*)(w + at.codes_b);
    unsigned *order_a = (unsigned*)(w + at.order_a), *order_b = (unsigned*)(w + at.order_b);
    Vec* sorted = (Vec*)(w + at.sorted);
    Bounds<T> *part = (Bounds<T>*)(w + at.part), *boxes = (Bounds<T>*)(w + at.boxes);
    const int nbox = (int)((nn + kBox - 1) / kBox), blocks = (n + kThreads - 1) / kThreads;
    // 1. bounding box of the cloud (two levels, fixed order)
    SYN3R_LAUNCH_NAMED(Scalar<T>::aabb, k_aabb<T>, dim3(nbox), dim3(kThreads), 0, stream, points, 3, n, kBox, part);
    SYN3R_LAUNCH_NAMED(Scalar<T>::aabb_final, k_aabb_final<T>, dim3(1), dim3(kThreads), 0, stream, part, nbox, boxes + nbox);
    // 2. Morton order (stable argsort of the 30-bit codes)
    SYN3R_LAUNCH_NAMED(Scalar<T>::morton, k_morton<T>, dim3(blocks), dim3(kThreads), 0, stream, points, n, boxes + nbox, codes_a);
    int in_b = 0;
    int rc = argsort_depth_u32(codes_a, order_a, codes_b, order_b, nn, w + at.sort_ws, stream, &in_b);
    if (rc != SYN3R_OK) return rc;
    const unsigned* order = in_b ? order_b : order_a;
    // 3. points in that order, bounds of every 1024 of them
    SYN3R_LAUNCH_NAMED(Scalar<T>::gather, k_gather<T>, dim3(blocks), dim3(kThreads), 0, stream, points, order, n, sorted);
    SYN3R_LAUNCH_NAMED(Scalar<T>::aabb, k_aabb<T>, dim3(nbox), dim3(kThreads), 0, stream, (const T*)sorted, 4, n, kBox, boxes);
    *out = {sorted, order, boxes, nbox, blocks};
    return SYN3R_OK;
}

}  // namespace

extern "C" size_t syn3r_pcd_outlier_workspace_bytes(int n) { return SYN3R_DIM_OK(n) ? Layout<double>((size_t)n).bytes : 0; }

extern "C" int syn3r_pcd_statistical_outlier(const double* points, int n, int nb_neighbors, double std_ratio, double* avg_dist,
                                             unsigned char* keep, double* stats, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(points && avg_dist && keep && stats && ws, "pcd_statistical_outlier: null pointer");
    SYN3R_REQUIRE(n >= 2 && n <= SYN3R_DIM_MAX, "pcd_statistical_outlier: needs 2 .. %d points, got %d", SYN3R_DIM_MAX, n);
    SYN3R_REQUIRE(nb_neighbors == 20, "pcd_statistical_outlier: built for nb_neighbors = 20 (model/diffusionGS.py:321), got %d",
                  nb_neighbors);
    SYN3R_REQUIRE(std_ratio > 0.0, "pcd_statistical_outlier: std_ratio must be positive");
    hipStream_t stream = (hipStream_t)stream_;
    Prepared<double> s;
    if (int rc = prepare("pcd_statistical_outlier", points, n, ws, ws_bytes, SYN3R_E_INVALID, stream, &s)) return rc;
    SYN3R_LAUNCH(k_knn_mean64<20>, dim3(s.blocks), dim3(kThreads), 0, stream, s.sorted, s.order, s.boxes, n, s.nbox, avg_dist);
    SYN3R_LAUNCH(k_outlier_stats, dim3(1), dim3(1024), 0, stream, avg_dist, n, std_ratio, stats);
    SYN3R_LAUNCH(k_outlier_keep, dim3(s.blocks), dim3(kThreads), 0, stream, avg_dist, n, stats, keep);
    SYN3R_LAUNCH_CHECK("pcd_statistical_outlier");
    return SYN3R_OK;
}

extern "C" size_t syn3r_knn3_workspace_bytes(int n) { return SYN3R_DIM_OK(n) ? Layout<float>((size_t)n).bytes : 0; }

extern "C" int syn3r_knn3_mean_dist2(const float* points, int n, float* out, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(points && out && ws, "knn3: null pointer");
    SYN3R_REQUIRE(n >= 4 && n <= SYN3R_DIM_MAX, "knn3: needs 4 .. %d points (3 neighbours), got %d", SYN3R_DIM_MAX, n);
    hipStream_t stream = (hipStream_t)stream_;
    Prepared<float> s;
    if (int rc = prepare("knn3", points, n, ws, ws_bytes, SYN3R_E_INVALID, stream, &s)) return rc;
    SYN3R_LAUNCH(k_knn3, dim3(s.blocks), dim3(kThreads), 0, stream, s.sorted, s.order, s.boxes, n, s.nbox, out);
    SYN3R_LAUNCH_CHECK("knn3");
    return SYN3R_OK;
}

extern "C" size_t syn3r_knn3_graph_workspace_bytes(int n) { return syn3r_knn3_workspace_bytes(n); }      // the same layout

extern "C" int syn3r_knn3_graph(const float* points, int n, float* dist2, int* index, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(points && dist2 && index && ws, "knn3_graph: null pointer");
    SYN3R_REQUIRE(n >= 4 && n <= SYN3R_DIM_MAX, "knn3_graph: needs 4 .. %d points (3 neighbours), got n=%d", SYN3R_DIM_MAX, n);
    hipStream_t stream = (hipStream_t)stream_;
    Prepared<float> s;
    if (int rc = prepare("knn3_graph", points, n, ws, ws_bytes, SYN3R_E_WORKSPACE, stream, &s)) return rc;
    SYN3R_LAUNCH(k_knn3_graph, dim3(s.blocks), dim3(kThreads), 0, stream, s.sorted, s.boxes, n, s.nbox, dist2, index);
    SYN3R_LAUNCH_CHECK("knn3_graph");
    return SYN3R_OK;
}

extern "C" size_t syn3r_gaussian_unpool_workspace_bytes(int n) {
    if (!SYN3R_DIM_OK(n)) return 0;
    const size_t nblk = ((size_t)n + kThreads - 1) / kThreads;
    return align256(nblk * 4) * 2 + align256((size_t)n) + 256;      // block counts, block offsets, flags
}

extern "C" int syn3r_gaussian_unpool_count(const float* dist2, const float* log_scales, int n, float score_thresh,
                                           float log_scale_thresh, int* count, void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(dist2 && log_scales && count && ws, "gaussian_unpool_count: null pointer");
    SYN3R_REQUIRE(n >= 4 && n <= SYN3R_DIM_MAX, "gaussian_unpool_count: needs 4 .. %d Gaussians, got n=%d", SYN3R_DIM_MAX, n);
    SYN3R_REQUIRE(score_thresh == score_thresh && log_scale_thresh == log_scale_thresh, "gaussian_unpool_count: NaN threshold");
    if (int rc = ws_check("gaussian_unpool_count", ws, ws_bytes, syn3r_gaussian_unpool_workspace_bytes(n), SYN3R_E_WORKSPACE)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int nblk = (n + kThreads - 1) / kThreads;
    char* w = (char*)ws;
    int* counts = (int*)w; w += align256((size_t)nblk * 4);
    int* offsets = (int*)w; w += align256((size_t)nblk * 4);
    unsigned char* flags = (unsigned char*)w;
    SYN3R_LAUNCH(k_unpool_flag, dim3(nblk), dim3(kThreads), 0, stream, dist2, log_scales, n, score_thresh, log_scale_thresh, flags, counts);
    SYN3R_LAUNCH(k_unpool_scan, dim3(1), dim3(kThreads), 0, stream, (const int*)counts, nblk, offsets, count);
    SYN3R_LAUNCH_CHECK("gaussian_unpool_count");
    return SYN3R_OK;
}

extern "C" int syn3r_gaussian_unpool_emit(const float* xyz, const float* log_scales, const float* opacity_logits,
                                          const float* confidence, const int* index, int n, int n_sources, int capacity,
                                          float* out_xyz, float* out_log_scales, float* out_opacity_logits, float* out_rotations,
                                          float* out_confidence, const void* ws, size_t ws_bytes, void* stream_) {
    SYN3R_REQUIRE(xyz && log_scales && opacity_logits && confidence && index && ws, "gaussian_unpool_emit: null pointer");
    SYN3R_REQUIRE(out_xyz && out_log_scales && out_opacity_logits && out_rotations && out_confidence,
                  "gaussian_unpool_emit: null pointer (output)");
    SYN3R_REQUIRE(n >= 4 && n <= SYN3R_DIM_MAX, "gaussian_unpool_emit: needs 4 .. %d Gaussians, got n=%d", SYN3R_DIM_MAX, n);
    SYN3R_REQUIRE(n_sources >= 0 && n_sources <= n, "gaussian_unpool_emit: n_sources=%d outside 0 .. n=%d", n_sources, n);
    SYN3R_REQUIRE(capacity >= 0 && (long long)capacity >= 3ll * n_sources,
                  "gaussian_unpool_emit: capacity of %d rows is too small for 3 x %d new Gaussians", capacity, n_sources);
    if (int rc = ws_check("gaussian_unpool_emit", ws, ws_bytes, syn3r_gaussian_unpool_workspace_bytes(n), SYN3R_E_WORKSPACE)) return rc;
    SYN3R_REQUIRE(((uintptr_t)out_rotations & 15) == 0, "gaussian_unpool_emit: out_rotations must be 16-byte aligned");
    if (n_sources == 0) return SYN3R_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const int nblk = (n + kThreads - 1) / kThreads;
    const char* w = (const char*)ws;
    w += align256((size_t)nblk * 4);
    const int* offsets = (const int*)w; w += align256((size_t)nblk * 4);
    const unsigned char* flags = (const unsigned char*)w;
    SYN3R_LAUNCH(k_unpool_emit, dim3(nblk), dim3(kThreads), 0, stream, xyz, log_scales, opacity_logits, confidence, index, n, flags,
                 offsets, capacity, out_xyz, out_log_scales, out_opacity_logits, out_rotations, out_confidence);
    SYN3R_LAUNCH_CHECK("gaussian_unpool_emit");
    return SYN3R_OK;
}
