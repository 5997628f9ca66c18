// Single-call UNet forward at the C-ABI: syn3r_unet_create / _workspace_bytes / _forward / _destroy.
//
// What SURVEY.md 8(b) lists for hosts that are not Python: `self.unet(latent_model_input, t, encoder_hidden_states=...,
// added_time_ids=..., return_dict=False)[0]` (model/SVD_2pass_prob_uncertain_post.py:763,786;
// diffusers/models/unets/unet_spatio_temporal_condition.py:356-489) as ONE call on device pointers, with the weights read
// from a diffusers checkpoint directory (`from_pretrained(<local dir>, torch_dtype=float16, variant="fp16")`,
// model/diffusionGS.py:1089).  This file is the launch graph only - the same launch sequence, on the same operators of this
// library (gemm.hip, attn.hip, norm.hip), that syn3r_amd/unet/model.py issues from Python: the upload of what the checkpoint
// reader (unet_ckpt.hip: config.json, safetensors, weight repacking - host code, no device) hands over, a stream-ordered
// arena over the caller's workspace, and the block loops of unet_3d_blocks.py / transformer_temporal.py / resnet.py.
// The handful of elementwise steps the Python host leaves to torch (sinusoidal embeddings, SiLU on [B, 1280] vectors,
// NCHW <-> NHWC at the two ends) are small kernels at the top of the file.
#include "common.h"
#include "unet_ckpt.h"
#include <exception>
#include <map>
#include <memory>
#include <algorithm>
#include <unordered_set>
#include <mutex>

using namespace syn3r;

namespace {

// ------------------------------------------------------------------------------------------------ glue kernels
// embeddings.py Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): [cos | sin] of t * exp(-ln(1e4) i / half),
// fp32 arithmetic in the order model.py:timestep_embedding spells it, rounded to fp16 at the end.
__global__ void k_timestep_embedding(const float* __restrict__ t_dev, double t_host, float t_step, int n, int dim, __half* __restrict__ out) {
    const int half = dim / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * half) return;
    const int r = i / half, c = i - r * half;
    const float t = t_dev ? t_dev[r] : (float)t_host + t_step * (float)r;
    // (`tensor / python_int` on the device is a multiplication by the fp32 reciprocal in torch: the same here, or the two hosts
    // differ in the last bit of the exponent whenever `half` is not a power of two)
    const float e = expf((-9.210340371976184f * (float)c) * (1.0f / (float)half));
    const float a = t * e;
    out[(size_t)r * dim + c] = __float2half(cosf(a));
    out[(size_t)r * dim + half + c] = __float2half(sinf(a));
}
__global__ void k_silu(const __half* __restrict__ x, __half* __restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = __half2float(x[i]);
    y[i] = __float2half(v / (1.0f + expf(-v)));
}
__global__ void k_add(const __half* __restrict__ a, const __half* __restrict__ b, __half* __restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __float2half(__half2float(a[i]) + __half2float(b[i]));
}
// [N, C, h, w] -> [N, h, w, CP] (channels zero-padded to CP)
__global__ void k_nchw_to_nhwc(const __half* __restrict__ x, __half* __restrict__ y, int N, int C, int hw, int CP) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * hw * CP) return;
    const int c = (int)(i % CP);
    const long long pix = i / CP;
    const int n = (int)(pix / hw), p = (int)(pix - (long long)n * hw);
    y[i] = c < C ? x[((long long)n * C + c) * hw + p] : __float2half(0.f);
}
// [N, h, w, CP] -> [N, C, h, w] (the first C channels)
__global__ void k_nhwc_to_nchw(const __half* __restrict__ x, __half* __restrict__ y, int N, int C, int hw, int CP) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * C * hw) return;
    const int p = (int)(i % hw);
    const long long nc = i / hw;
    const int n = (int)(nc / C), c = (int)(nc - (long long)n * C);
    y[i] = x[((long long)n * hw + p) * CP + c];
}
// y[r] = x[r % rows_in]  (e.repeat(B, 1))
__global__ void k_repeat_rows(const __half* __restrict__ x, __half* __restrict__ y, int rows_in, long long rows_out, int C) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows_out * C) return;
    const long long r = i / C;
    y[i] = x[(r % rows_in) * C + (i - r * C)];
}
// [x1 | x2] along the channels (the fallback of the two-source contraction)
__global__ void k_cat_cols(const __half* __restrict__ a, int C1, const __half* __restrict__ b, int C2, __half* __restrict__ y, long long M) {
    const int C = C1 + C2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * C) return;
    const long long r = i / C;
    const int c = (int)(i - r * C);
    y[i] = c < C1 ? a[r * C1 + c] : b[r * C2 + (c - C1)];
}

// ------------------------------------------------------------------------------------------------ model
struct Wt { __half* p = nullptr; long long rows = 0, cols = 0; };       // a packed device tensor ([rows, cols], cols = the rest)

}  // namespace

struct syn3r_unet : Checkpoint {                                        // the plan, alpha and temb_slice as read; `packs` is emptied once uploaded
    int device = 0;
    char* blob = nullptr; size_t blob_bytes = 0;                        // every packed weight, one allocation
    std::unordered_map<std::string, Wt> w;
    struct PosEmb { __half* p = nullptr; hipEvent_t ready = nullptr; hipStream_t stream = nullptr; };
    std::map<std::string, PosEmb> pos_cache;                            // frame-position embeddings per (block, F, B): functions of the weights only
    bool ff_ln = true, ln_qkv = true;
};

namespace {

// Live handles: every entry point checks its handle against this set (a stale or fabricated pointer is an error, not a crash).
std::mutex g_unet_mu;
std::unordered_set<const syn3r_unet*>& unet_registry() { static auto* s = new std::unordered_set<const syn3r_unet*>; return *s; }
bool unet_live(const syn3r_unet* m) {
    std::lock_guard<std::mutex> lk(g_unet_mu);
    return m && unet_registry().count(m);
}

int unet_create_impl(const char* weights_dir, const char* variant, syn3r_unet** out) {
    std::unique_ptr<syn3r_unet> m(new syn3r_unet);
    int rc = load_checkpoint(weights_dir, variant, *m);
    if (rc) return rc;
    rc = check_hip(hipGetDevice(&m->device), "hipGetDevice");
    if (rc) return rc;
    size_t total = 0;
    for (auto& hp : m->packs) total += (hp.d.size() * 2 + 255) / 256 * 256;
    rc = check_hip(hipMalloc((void**)&m->blob, total ? total : 256), "hipMalloc(unet weights)");
    if (rc) return rc;
    m->blob_bytes = total;
    size_t off = 0;
    for (auto& hp : m->packs) {
        rc = check_hip(hipMemcpy(m->blob + off, hp.d.data(), hp.d.size() * 2, hipMemcpyHostToDevice), "hipMemcpy(unet weights)");
        if (rc) { (void)hipFree(m->blob); return rc; }
        m->w[hp.name] = Wt{(__half*)(m->blob + off), hp.rows, hp.cols};
        off += (hp.d.size() * 2 + 255) / 256 * 256;
    }
    std::vector<HostPack>().swap(m->packs);                // the host copies are on the device now
    m->ff_ln = tune_env("SYN3R_FF_LN", 1) != 0;          // tuning builds only (common.h): the shipped library reads no environment
    m->ln_qkv = tune_env("SYN3R_LN_QKV", 1) != 0;
    *out = m.release();
    {
        std::lock_guard<std::mutex> lk(g_unet_mu);
        unet_registry().insert(*out);
    }
    return SYN3R_OK;
}

}  // namespace

// The reader parses files it does not control (config.json, the safetensors header): nothing may leave through extern "C" as a
// C++ exception (bad_alloc / length_error from a hostile header would terminate a ctypes / cgo host).
extern "C" int syn3r_unet_create(const char* weights_dir, const char* variant, syn3r_unet** out) {
    SYN3R_REQUIRE(weights_dir && out, "unet_create: null argument");
    *out = nullptr;
    try {
        return unet_create_impl(weights_dir, variant, out);
    } catch (const std::exception& e) {
        set_error("unet_create: %s", e.what());
    } catch (...) {
        set_error("unet_create: unexpected exception");
    }
    *out = nullptr;
    return SYN3R_E_INVALID;
}

extern "C" int syn3r_unet_destroy(syn3r_unet* m) {
    if (!m) return SYN3R_OK;
    {
        std::lock_guard<std::mutex> lk(g_unet_mu);
        if (!unet_registry().erase(m)) { set_error("unet_destroy: not a live handle"); return SYN3R_E_INVALID; }
    }
    for (auto& kv : m->pos_cache) {
        if (kv.second.ready) (void)hipEventDestroy(kv.second.ready);
        (void)hipFree(kv.second.p);
    }
    if (m->blob) (void)hipFree(m->blob);
    delete m;
    return SYN3R_OK;
}

// ================================================================================================ forward
namespace {

// Stream-ordered arena over the caller's workspace: first-fit with coalescing.  Every kernel of a forward runs on ONE stream,
// so a block may be handed out again as soon as the host has ENQUEUED its last reader (what a caching allocator does for
// one stream).  In `dry` mode nothing is launched and only the high-water mark is tracked: the same allocation sequence as
// the real run, so syn3r_unet_workspace_bytes is exact.
struct Arena {
    char* base = nullptr; size_t cap = 0, peak = 0;
    std::map<size_t, size_t> free_;        // offset -> size
    std::unordered_map<size_t, size_t> live;
    void reset(char* b, size_t c) { base = b; cap = c; peak = 0; free_.clear(); live.clear(); free_[0] = c; }
    void* alloc(size_t n) {
        n = (n + 255) / 256 * 256;
        if (!n) n = 256;
        for (auto it = free_.begin(); it != free_.end(); ++it) {
            if (it->second >= n) {
                const size_t off = it->first, rest = it->second - n;
                free_.erase(it);
                if (rest) free_[off + n] = rest;
                live[off] = n;
                peak = std::max(peak, off + n);
                return base + off;
            }
        }
        return nullptr;
    }
    void release(void* p) {
        if (!p) return;
        size_t off = (size_t)((char*)p - base);
        auto it = live.find(off);
        if (it == live.end()) return;
        size_t n = it->second;
        live.erase(it);
        auto nx = free_.lower_bound(off);
        if (nx != free_.end() && off + n == nx->first) { n += nx->second; nx = free_.erase(nx); }
        if (nx != free_.begin()) {
            auto pv = std::prev(nx);
            if (pv->first + pv->second == off) { pv->second += n; return; }
        }
        free_[off] = n;
    }
};

// an activation [rows, cols] in the arena; gnp: the GroupNorm partial sums its producer was asked for (the gn_partials argument of
// the contractions), gn_ok: the kernel that ran wrote them (their gn_written answer)
struct T { __half* p = nullptr; long long rows = 0; int cols = 0; float* gnp = nullptr; int gn_ok = 0; };

struct Epi {                                                              // the fused epilogue of syn3r_gemm_f16 and friends
    const __half* rowvec = nullptr; long long ldrv = 0; int rows_per_vec = 0, rv_group = 0;
    const T* residual = nullptr; const T* aux = nullptr;
    float s_acc = 1.f, s_res = 1.f, s_aux = 1.f;
    const __half* res_p() const { return residual ? residual->p : nullptr; }
    int res_ld() const { return residual ? residual->cols : 0; }
    int res_ld(int ld) const { return residual ? ld : 0; }               // (conv3x3 / tconv3 name the output's width)
    const __half* aux_p() const { return aux ? aux->p : nullptr; }
    int aux_ld() const { return aux ? aux->cols : 0; }
};

struct Run {
    syn3r_unet& m;
    Arena ar;
    bool dry = false;
    hipStream_t stream = nullptr;
    int B, F, h, w, G;                              // G: the context group (it changes epilogue arguments, not buffers)
    bool shared_ctx;
    T ehs, temb_all;
    std::unordered_map<std::string, T> cross;      // folded cross-attention vectors of this forward
    int rc = SYN3R_OK;
    Run(syn3r_unet& m_, int B_, int F_, int h_, int w_, int G_, int ehs_rows) : m(m_), B(B_), F(F_), h(h_), w(w_), G(G_), shared_ctx(B_ == 1 || ehs_rows == 1) {}

    const Wt* W(const std::string& k) {
        auto it = m.w.find(k);
        if (it == m.w.end()) { if (!rc) { set_error("unet_forward: the checkpoint has no tensor %s", k.c_str()); rc = SYN3R_E_INVALID; } return nullptr; }
        return &it->second;
    }
    const __half* Wp(const std::string& k) { const Wt* t = W(k); return t ? t->p : nullptr; }
    bool ok() const { return rc == SYN3R_OK; }
    // every buffer of a forward comes from the arena through here (nothing after the first error)
    void* take(size_t bytes) {
        void* p = ok() ? ar.alloc(bytes) : nullptr;
        if (ok() && !p) { set_error("unet_forward: workspace too small (needs syn3r_unet_workspace_bytes)"); rc = SYN3R_E_WORKSPACE; }
        return p;
    }
    T make(long long rows, int cols) {
        T t; t.rows = rows; t.cols = cols; t.p = (__half*)take((size_t)rows * cols * 2);
        return t;
    }
    void drop(T& t) { ar.release(t.p); t.p = nullptr; ar.release(t.gnp); t.gnp = nullptr; t.gn_ok = 0; }
    // GroupNorm statistics from the producer's epilogue (model.py: gn_stats=TUNE["gn_epilogue"]): the buffer is part of the
    // allocation sequence whenever the shape can carry partial sums (dry runs see the same sequence); whether the kernel chosen
    // for the shape wrote them is the launch's answer (out.gn_ok).  Returns the size of out.gnp.
    size_t gn_begin(T& out, bool want) {
        static const int gn_env = tune_env("SYN3R_GN_EPILOGUE", 1);
        const size_t nb = (want && gn_env != 0 && out.rows <= SYN3R_DIM_MAX) ? syn3r_gn_partials_bytes((int)out.rows, out.cols) : 0;
        if (!nb || !ok()) return 0;
        out.gnp = (float*)take(nb);
        return out.gnp ? nb : 0;
    }
    void chk(int r) { if (r && !rc) rc = r; }
    bool go() const { return ok() && !dry; }
    // a glue kernel over n elements, one thread each
    template <class K, class... A> void launch1d(K kernel, long long n, A... args) {
        if (go()) hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, args...);
    }

    // ---- operators (ops.py)
    T linear(const T& x, long long ldx, int K, const std::string& wname, const char* bias_name, const Epi& e = Epi(), bool gn = false) {
        const Wt* wt = W(wname);
        const __half* b = bias_name ? Wp(bias_name) : nullptr;
        T out = make(x.rows, wt ? (int)wt->rows : 0);
        const size_t gnb = gn_begin(out, gn);
        if (go())
            chk(syn3r_gemm_f16(x.p, ldx, wt->p, out.p, out.cols, b, e.rowvec, e.ldrv, e.rows_per_vec, e.rv_group,
                               e.res_p(), e.res_ld(), e.aux_p(), e.aux_ld(), e.s_acc, e.s_res, e.s_aux, (int)x.rows, out.cols, K, out.gnp, gnb, &out.gn_ok, stream));
        return out;
    }
    T linear(const T& x, const std::string& wname, const std::string& bname, const Epi& e = Epi(), bool gn = false) {
        return linear(x, x.cols, x.cols, wname, bname.empty() ? nullptr : bname.c_str(), e, gn);
    }
    T linear_cat(const T& x1, const T& x2, const std::string& wname, const std::string& bname) {
        const Wt* wt = W(wname);
        const int N = wt ? (int)wt->rows : 0;
        if (ok() && syn3r_gemm_2src_supported((int)x1.rows, N, x1.cols, x2.cols, x1.cols, x2.cols)) {
            T out = make(x1.rows, N);
            if (go()) chk(syn3r_gemm_2src_f16(x1.p, x1.cols, x1.cols, x2.p, x2.cols, x2.cols, wt->p, out.p, N, Wp(bname), (int)x1.rows, N, nullptr, 0, nullptr, stream));
            return out;
        }
        T cat = make(x1.rows, x1.cols + x2.cols);
        launch1d(k_cat_cols, cat.rows * cat.cols, x1.p, x1.cols, x2.p, x2.cols, cat.p, cat.rows);
        T out = linear(cat, wname, bname);
        drop(cat);
        return out;
    }
    T conv3x3(const T& x, int NB, int Hi, int Wi, int Cin, const std::string& wname, const std::string& bname, int stride, bool ups,
              const Epi& e, int* Ho_ = nullptr, int* Wo_ = nullptr, bool gn = true) {
        const Wt* wt = W(wname);
        const int Cout = wt ? (int)wt->rows : 0;
        const int Hg = ups ? 2 * Hi : Hi, Wg = ups ? 2 * Wi : Wi;
        const int Ho = (Hg + 1 - 2) / stride + 1, Wo = (Wg + 1 - 2) / stride + 1;
        if (Ho_) *Ho_ = Ho;
        if (Wo_) *Wo_ = Wo;
        T out = make((long long)NB * Ho * Wo, Cout);
        const size_t gnb = gn_begin(out, gn);
        if (go())
            chk(syn3r_conv2d3x3_f16(x.p, wt->p, out.p, Cout, Wp(bname), e.rowvec, e.ldrv, e.rows_per_vec, e.res_p(), e.res_ld(Cout), e.s_acc, e.s_res, NB, Hi, Wi, Cin, Cout, stride, ups ? 1 : 0, 1, out.gnp, gnb, &out.gn_ok, stream));
        return out;
    }
    // nearest-2x upsample + 3x3 convolution in its four-phase form (ops.conv3x3_up4; weights folded by pack_weights)
    T conv3x3_up4(const T& x, int NB, int Hi, int Wi, int Cin, const std::string& wname, const std::string& bname, int* Ho_, int* Wo_) {
        const Wt* wt = W(wname + "_up4");
        const int Cout = wt ? (int)(wt->rows / 4) : 0;
        *Ho_ = 2 * Hi; *Wo_ = 2 * Wi;
        T out = make((long long)NB * 4 * Hi * Wi, Cout);
        const size_t gnb = gn_begin(out, true);
        if (go()) chk(syn3r_conv2d3x3_up4_f16(x.p, wt->p, out.p, Wp(bname), nullptr, NB, Hi, Wi, Cin, Cout, out.gnp, gnb, &out.gn_ok, stream));
        return out;
    }
    T tconv3(const T& x, const std::string& wname, const std::string& bname, int HW, const Epi& e) {
        const Wt* wt = W(wname);
        const int Cout = wt ? (int)wt->rows : 0;
        T out = make(x.rows, Cout);
        const size_t gnb = gn_begin(out, true);  // (every temporal convolution's output is a GroupNorm input, model.py:_resblock)
        if (go())
            chk(syn3r_tconv3_f16(x.p, wt->p, out.p, Cout, Wp(bname), e.rowvec, e.ldrv, e.rows_per_vec, e.res_p(), e.res_ld(Cout), e.s_acc, e.s_res, B, F, HW, x.cols, Cout, out.gnp, gnb, &out.gn_ok, stream));
        return out;
    }
    T groupnorm(const T& x, const std::string& pre, int samples, float eps, bool silu, const T* x2 = nullptr) {
        const int rows = (int)(x.rows / samples);
        const size_t wsb = syn3r_groupnorm_workspace_bytes(samples, rows);
        const int Ct = x.cols + (x2 ? x2->cols : 0);
        T out = make(x.rows, Ct);
        void* ws = take(wsb);
        if (go() && x.gn_ok && (!x2 || x2->gn_ok) && rows % 32 == 0 && Ct % 320 == 0 && x.cols % 10 == 0) {      // ops.py:groupnorm, the same rule
            chk(syn3r_groupnorm_pre_f16(x.p, x.cols, x.gnp, x2 ? x2->p : nullptr, x2 ? x2->cols : 0, x2 ? x2->gnp : nullptr, out.p, samples, rows,
                                        Wp(pre + ".weight"), Wp(pre + ".bias"), eps, silu, ws, wsb, stream));
        } else if (go()) {
            if (x2) chk(syn3r_groupnorm_2src_f16(x.p, x.cols, x2->p, x2->cols, out.p, samples, rows, Wp(pre + ".weight"), Wp(pre + ".bias"), eps, silu, ws, wsb, stream));
            else chk(syn3r_groupnorm_f16(x.p, out.p, samples, rows, x.cols, Wp(pre + ".weight"), Wp(pre + ".bias"), eps, silu, ws, wsb, stream));
        }
        ar.release(ws);
        return out;
    }
    // y = LayerNorm(x [+ addvec]); xsum (optional) receives x + addvec
    T layernorm(const T& x, const std::string& pre, const __half* addvec = nullptr, int rows_per_vec = 0, T* xsum = nullptr) {
        T out = make(x.rows, x.cols);
        if (xsum) *xsum = make(x.rows, x.cols);
        if (go())
            chk(syn3r_layernorm_f16(x.p, out.p, xsum ? xsum->p : nullptr, addvec, rows_per_vec, x.rows, x.cols, Wp(pre + ".weight"), Wp(pre + ".bias"), 1e-5f, stream));
        return out;
    }
    // model.py:_norm_qkv - attn1's stacked q / k / v projection of norm1(x): one kernel at C = 320
    T norm_qkv(const std::string& blk, const T& x) {
        const Wt* wq = W(blk + ".attn1.qkv");
        if (m.ln_qkv && x.cols == 320 && wq && wq->rows % 320 == 0) {
            T out = make(x.rows, (int)wq->rows);
            if (go())
                chk(syn3r_layernorm_linear320_f16(x.p, x.cols, Wp(blk + ".norm1.weight"), Wp(blk + ".norm1.bias"), 1e-5f, wq->p, out.p, out.cols,
                                                  (int)x.rows, (int)wq->rows, x.cols, stream));
            return out;
        }
        T n1 = layernorm(x, blk + ".norm1");
        T qkv = linear(n1, blk + ".attn1.qkv", "");
        drop(n1);
        return qkv;
    }
    T attention(const T& qkv, int nseq, int S, int heads) {
        const int C = heads * 64;
        T out = make(qkv.rows, C);
        if (go()) chk(syn3r_attention_f16(qkv.p, qkv.p + C, qkv.p + 2 * C, 3 * C, out.p, C, nseq, S, heads, stream));
        return out;
    }
    T attention_temporal(const T& qkv, int HW, int heads) {
        const int C = heads * 64;
        T out = make(qkv.rows, C);
        if (go()) chk(syn3r_attention_temporal_f16(qkv.p, qkv.p + C, qkv.p + 2 * C, 3 * C, out.p, C, B, F, HW, heads, stream));
        return out;
    }
    // model.py:_ff - FeedForward of block `pre` on x, `norm` = the LayerNorm in front of it (fused at C = 320)
    T ff(const std::string& pre, const T& x_in, const std::string& norm, const Epi& e) {
        const Wt* w0 = W(pre + ".net.0.proj.weight");
        const int D = w0 ? (int)(w0->rows / 2) : 0;
        const std::string w2 = pre + ".net.2.weight", b2 = pre + ".net.2.bias";
        T x = x_in;
        bool own = false;
        T out;
        if (m.w.count(pre + ".net.0.proj.geglu_cw")) {
            const bool fuse_ln = !norm.empty() && m.ff_ln;
            if (!norm.empty() && !fuse_ln) { x = layernorm(x_in, norm); own = true; }
            out = make(x.rows, x.cols);
            if (go()) {
                if (fuse_ln)
                    chk(syn3r_feedforward_fused_ln_f16(x.p, x.cols, Wp(norm + ".weight"), Wp(norm + ".bias"), 1e-5f, Wp(pre + ".net.0.proj.geglu_cw"),
                                                       Wp(pre + ".net.0.proj.geglu_cb"), D, Wp(w2), Wp(b2), out.p, out.cols, e.res_p(), e.res_ld(), e.aux_p(), e.aux_ld(),
                                                       e.s_acc, e.s_res, e.s_aux, (int)x.rows, x.cols, stream));
                else
                    chk(syn3r_feedforward_fused_f16(x.p, x.cols, Wp(pre + ".net.0.proj.geglu_cw"), Wp(pre + ".net.0.proj.geglu_cb"), D, Wp(w2), Wp(b2),
                                                    out.p, out.cols, e.res_p(), e.res_ld(), e.aux_p(), e.aux_ld(), e.s_acc, e.s_res, e.s_aux, (int)x.rows, x.cols, stream));
            }
        } else {
            if (!norm.empty()) { x = layernorm(x_in, norm); own = true; }
            const Wt* wt2 = W(w2);
            const int N = wt2 ? (int)wt2->rows : 0;
            out = make(x.rows, N);
            const size_t wsb = syn3r_feedforward_workspace_bytes((int)x.rows, D);
            void* ws = take(wsb);
            // model.py:_ff - net.0 on the 256 x 256 tile where the shape has whole tiles (bit-identical to the 80-column path)
            static const int g256_env = tune_env("SYN3R_FF_G256", 1);
            const bool p64 = g256_env != 0 && m.w.count(pre + ".net.0.proj.geglu_w64") && syn3r_feedforward_p64_supported((int)x.rows, D, x.cols);
            if (go() && p64)
                chk(syn3r_feedforward_p64_f16(x.p, x.cols, Wp(pre + ".net.0.proj.geglu_w64"), Wp(pre + ".net.0.proj.geglu_b64"), D, Wp(w2), Wp(b2), out.p, N,
                                              e.res_p(), e.res_ld(), e.aux_p(), e.aux_ld(), e.s_acc, e.s_res, e.s_aux, (int)x.rows, x.cols, N, ws, wsb, stream));
            else if (go())
                chk(syn3r_feedforward_f16(x.p, x.cols, Wp(pre + ".net.0.proj.geglu_w"), Wp(pre + ".net.0.proj.geglu_b"), D, Wp(w2), Wp(b2), out.p, N,
                                          e.res_p(), e.res_ld(), e.aux_p(), e.aux_ld(), e.s_acc, e.s_res, e.s_aux, (int)x.rows, x.cols, N, ws, wsb, stream));
            ar.release(ws);
        }
        if (own) drop(x);
        return out;
    }
    T silu(const T& x) {
        T y = make(x.rows, x.cols);
        launch1d(k_silu, x.rows * x.cols, x.p, y.p, x.rows * x.cols);
        return y;
    }
    // TimestepEmbedding (embeddings.py): linear_2(silu(linear_1(x))); x is released as soon as linear_1 has read it
    T embed_mlp(const std::string& pre, T& x) {
        T a = linear(x, pre + ".linear_1.weight", pre + ".linear_1.bias");
        drop(x);
        T s = silu(a);
        drop(a);
        T o = linear(s, pre + ".linear_2.weight", pre + ".linear_2.bias");
        drop(s);
        return o;
    }
    // attn2 with a single key: to_out(to_v(ctx)) per context row (model.py:_cross_vec); kept for the forward
    const T& cross_vec(const std::string& pre) {
        auto it = cross.find(pre);
        if (it != cross.end()) return it->second;
        T v = linear(ehs, pre + ".to_v.weight", "");
        T o = linear(v, pre + ".to_out.0.weight", pre + ".to_out.0.bias");
        drop(v);
        return cross.emplace(pre, o).first->second;
    }

    // AlphaBlender scales of `pre`.time_mixer: (alpha, 1 - alpha), model.py:_blend_scales
    void blend(const std::string& pre, double& a, double& om) {
        auto al = m.alpha.find(pre + ".time_mixer.mix_factor");
        a = al != m.alpha.end() ? al->second.first : 0.5; om = al != m.alpha.end() ? al->second.second : 0.5;
        if (al == m.alpha.end() && !rc) { set_error("unet_forward: the checkpoint has no %s.time_mixer.mix_factor", pre.c_str()); rc = SYN3R_E_INVALID; }
    }

    // SpatioTemporalResBlock (resnet.py:325-378, 613-636, 789-802); x2: the block input is [x | x2] (up blocks)
    T resblock(const std::string& pre, const T& x, int cin, int cout, const T* x2) {
        const int HW = h * w;
        const std::string s = pre + ".spatial_res_block", t = pre + ".temporal_res_block";
        auto slice = [&](const std::string& name, Epi& e) {
            auto it = m.temb_slice.find(name);
            e.rowvec = temb_all.p ? temb_all.p + (it != m.temb_slice.end() ? it->second.first : 0) : nullptr;
            if (dry) e.rowvec = nullptr;
            e.ldrv = temb_all.cols; e.rows_per_vec = F * HW;
        };
        T h1 = groupnorm(x, s + ".norm1", B * F, 1e-5f, true, x2);
        Epi e1; slice(s + ".time_emb_proj", e1);
        T h2 = conv3x3(h1, B * F, h, w, cin, s + ".conv1.weight", s + ".conv1.bias", 1, false, e1);
        drop(h1);
        T h3 = groupnorm(h2, s + ".norm2", B * F, 1e-5f, true);
        drop(h2);
        T skip = x;
        bool own_skip = false;
        if (x2) { skip = linear_cat(x, *x2, s + ".conv_shortcut.weight", s + ".conv_shortcut.bias"); own_skip = true; }
        else if (cin != cout) { skip = linear(x, s + ".conv_shortcut.weight", s + ".conv_shortcut.bias"); own_skip = true; }
        Epi e2; e2.residual = &skip;
        T xs = conv3x3(h3, B * F, h, w, cout, s + ".conv2.weight", s + ".conv2.bias", 1, false, e2);
        drop(h3);
        if (own_skip) drop(skip);
        T g1 = groupnorm(xs, t + ".norm1", B, 1e-5f, true);
        Epi e3; slice(t + ".time_emb_proj", e3);
        T c1 = tconv3(g1, t + ".conv1.weight", t + ".conv1.bias", HW, e3);
        drop(g1);
        T g2 = groupnorm(c1, t + ".norm2", B, 1e-5f, true);
        drop(c1);
        double a, om;
        blend(pre, a, om);
        Epi e4; e4.residual = &xs; e4.s_acc = (float)om; e4.s_res = (float)(a + om);     // alpha xs + (1 - alpha)(xs + conv2)
        T out = tconv3(g2, t + ".conv2.weight", t + ".conv2.bias", HW, e4);
        drop(g2);
        drop(xs);
        return out;
    }

    // frame-position embedding of block `pre` (transformer_temporal.py:326-337), one row per (b, f): a function of the weights, F, B
    const __half* pos_embedding(const std::string& pre, int ch) {
        const std::string key = pre + "|" + std::to_string(F) + "|" + std::to_string(B);
        auto it = m.pos_cache.find(key);
        if (it != m.pos_cache.end() && !dry) {
            // filled on the stream of the forward that created it: a forward on ANOTHER stream orders itself behind that fill
            // (the header's "nothing synchronises" holds for the host; this is a device-side dependency)
            if (it->second.stream != stream && it->second.ready) chk(check_hip(hipStreamWaitEvent(stream, it->second.ready, 0), "hipStreamWaitEvent(position embedding)"));
            return it->second.p;
        }
        T pos = make(F, ch);
        launch1d(k_timestep_embedding, F * (ch / 2), (const float*)nullptr, 0.0, 1.0f, F, ch, pos.p);
        T e2 = embed_mlp(pre + ".time_pos_embed", pos);
        __half* keep = nullptr;
        if (go()) {
            chk(check_hip(hipMalloc((void**)&keep, (size_t)B * F * ch * 2), "hipMalloc(position embedding)"));
            if (ok()) {
                launch1d(k_repeat_rows, (long long)B * F * ch, e2.p, keep, F, (long long)B * F, ch);
                syn3r_unet::PosEmb pe;
                pe.p = keep; pe.stream = stream;
                if (hipEventCreateWithFlags(&pe.ready, hipEventDisableTiming) == hipSuccess) {
                    if (hipEventRecord(pe.ready, stream) != hipSuccess) { (void)hipEventDestroy(pe.ready); pe.ready = nullptr; }
                } else pe.ready = nullptr;
                m.pos_cache[key] = pe;
            } else if (keep) { (void)hipFree(keep); keep = nullptr; }
        }
        drop(e2);
        return keep;
    }

    // TransformerSpatioTemporalModel (transformer_temporal.py:277-379) with its two blocks (attention.py:283-533)
    T transformer(const std::string& pre, const T& x, int ch, int heads) {
        const int HW = h * w;
        T gn = groupnorm(x, pre + ".norm", B * F, 1e-6f, false);
        T hs = linear(gn, pre + ".proj_in.weight", pre + ".proj_in.bias");
        drop(gn);
        const __half* emb = pos_embedding(pre, ch);
        const std::string b = pre + ".transformer_blocks.0", t = pre + ".temporal_transformer_blocks.0";
        {   // BasicTransformerBlock
            T qkv = norm_qkv(b, hs);
            T a1 = attention(qkv, B * F, HW, heads);
            drop(qkv);
            const T& cv = cross_vec(b + ".attn2");
            Epi e; e.residual = &hs; e.rowvec = dry ? nullptr : cv.p; e.ldrv = cv.cols; e.rows_per_vec = (shared_ctx ? B : 1) * F * HW;
            T o = linear(a1, b + ".attn1.to_out.0.weight", b + ".attn1.to_out.0.bias", e);
            drop(a1);
            drop(hs);
            hs = o;
            Epi ef; ef.residual = &hs;
            T f2 = ff(b + ".ff", hs, b + ".norm3", ef);
            drop(hs);
            hs = f2;
        }
        // TemporalBasicTransformerBlock on hs + emb
        T tt;
        if (m.ff_ln && m.w.count(t + ".ff_in.net.0.proj.geglu_cw")) {          // C = 320: add, norm_in, ff_in and + residual in one kernel
            tt = make(hs.rows, hs.cols);
            const Wt* w0 = W(t + ".ff_in.net.0.proj.weight");
            if (go())
                chk(syn3r_feedforward_fused_addln_f16(hs.p, hs.cols, emb, HW, Wp(t + ".norm_in.weight"), Wp(t + ".norm_in.bias"), 1e-5f,
                                                      Wp(t + ".ff_in.net.0.proj.geglu_cw"), Wp(t + ".ff_in.net.0.proj.geglu_cb"), w0 ? (int)(w0->rows / 2) : 0,
                                                      Wp(t + ".ff_in.net.2.weight"), Wp(t + ".ff_in.net.2.bias"), tt.p, tt.cols, nullptr, 0, 1.f, 1.f, 0.f,
                                                      (int)hs.rows, hs.cols, stream));
        } else {
            T hmix;
            T nin = layernorm(hs, t + ".norm_in", emb, HW, &hmix);
            Epi e0; e0.residual = &hmix;
            tt = ff(t + ".ff_in", nin, "", e0);
            drop(nin);
            drop(hmix);
        }
        {
            T qkv = norm_qkv(t, tt);
            T a1 = attention_temporal(qkv, HW, heads);
            drop(qkv);
            // the reference's batch-interleaved temporal context (transformer_temporal.py:310-317 vs attention.py:487-489): see model.py
            int rpv, grp;
            if (shared_ctx) { rpv = B * F * HW; grp = 0; }
            else if (G == 1) { rpv = F * HW; grp = 0; }
            else {
                if (HW % G && !rc) { set_error("unet_forward: the temporal cross-attention context interleave needs h*w divisible by the group size %d", G); rc = SYN3R_E_INVALID; }
                rpv = -G; grp = G != B ? G * F * HW : 0;
            }
            const T& cv = cross_vec(t + ".attn2");
            Epi e; e.residual = &tt; e.rowvec = dry ? nullptr : cv.p; e.ldrv = cv.cols; e.rows_per_vec = rpv; e.rv_group = grp;
            T o = linear(a1, t + ".attn1.to_out.0.weight", t + ".attn1.to_out.0.bias", e);
            drop(a1);
            drop(tt);
            tt = o;
        }
        double a, om;
        blend(pre, a, om);
        Epi em; em.residual = &tt; em.aux = &hs; em.s_acc = (float)om; em.s_res = (float)om; em.s_aux = (float)a;   // alpha hs + (1 - alpha)(ff + tt)
        T mix = ff(t + ".ff", tt, t + ".norm3", em);
        drop(tt);
        drop(hs);
        Epi eo; eo.residual = &x;
        T out = linear(mix, pre + ".proj_out.weight", pre + ".proj_out.bias", eo, true);
        drop(mix);
        return out;
    }

    // unet_spatio_temporal_condition.py:356-489
    void forward(const __half* sample, double timestep, const __half* ehs_in, int ehs_rows, const float* added_ids, __half* out) {
        // split-K scratch for the lowest level's convolutions (model.py:forward, the same rule): set for this forward, on this thread
        void* splitk = nullptr;
        {
            const int down = 1 << (m.boc.size() - 1);
            const long long m_low = (long long)B * F * (h / down) * (w / down);
            if (tune_env("SYN3R_SPLITK", 1) != 0 && ((m_low + 255) / 256) * ((m.boc.back() + 159) / 160) * 2 <= 256) {
                const size_t bytes = (size_t)4 * m_low * m.boc.back() * 4;
                splitk = take(bytes);
                if (go()) chk(syn3r_gemm_set_splitk_workspace(splitk, bytes));
            }
        }
        forward_body(sample, timestep, ehs_in, ehs_rows, added_ids, out);
        if (splitk) {
            if (!dry) syn3r_gemm_set_splitk_workspace(nullptr, 0);
            ar.release(splitk);
        }
    }
    void forward_body(const __half* sample, double timestep, const __half* ehs_in, int ehs_rows, const float* added_ids, __half* out) {
        const int c0 = m.boc[0];
        // 1. time (:385-418)
        T te = make(B, c0);
        launch1d(k_timestep_embedding, B * (c0 / 2), (const float*)nullptr, timestep, 0.0f, B, c0, te.p);
        T emb = embed_mlp("time_embedding", te);
        const int nid = m.proj_in / m.add_dim;                             // time ids per sample (3: fps, motion bucket, noise aug)
        T ta = make((long long)B * nid, m.add_dim);
        launch1d(k_timestep_embedding, B * nid * (m.add_dim / 2), added_ids, 0.0, 0.0f, B * nid, m.add_dim, ta.p);
        T ta2 = ta; ta2.rows = B; ta2.cols = nid * m.add_dim;              // reshape(B, -1)
        T aug = embed_mlp("add_embedding", ta2);
        T es = make(emb.rows, emb.cols);
        launch1d(k_add, es.rows * es.cols, emb.p, aug.p, es.p, es.rows * es.cols);
        drop(emb);
        drop(aug);
        T act = silu(es);
        drop(es);
        temb_all = linear(act, "time_emb_proj.all.weight", "time_emb_proj.all.bias");
        drop(act);
        ehs.p = (__half*)ehs_in; ehs.rows = ehs_rows; ehs.cols = m.cross[0];
        // 2. conv_in on NHWC with the channels padded to 64 (:428)
        const int CP = (m.in_ch + 63) / 64 * 64;
        T xin = make((long long)B * F * h * w, CP);
        launch1d(k_nchw_to_nhwc, xin.rows * CP, sample, xin.p, B * F, m.in_ch, h * w, CP);
        T x = conv3x3(xin, B * F, h, w, CP, "conv_in.weight", "conv_in.bias", 1, false, Epi());
        drop(xin);
        std::vector<T> skips{x};
        // 3. down (:432-449)
        for (auto& bp : m.down) {
            const std::string bpre = "down_blocks." + std::to_string(bp.idx);
            for (size_t j = 0; j < bp.layers.size(); ++j) {
                T y = resblock(bpre + ".resnets." + std::to_string(j), x, bp.layers[j].first, bp.layers[j].second, nullptr);
                if (bp.attn) { T z = transformer(bpre + ".attentions." + std::to_string(j), y, bp.layers[j].second, bp.heads); drop(y); y = z; }
                x = y;                                                     // (the previous x lives on in `skips`)
                skips.push_back(x);
            }
            if (bp.resample) {
                int Ho, Wo;
                T y = conv3x3(x, B * F, h, w, bp.ch, bpre + ".downsamplers.0.conv.weight", bpre + ".downsamplers.0.conv.bias", 2, false, Epi(), &Ho, &Wo);
                h = Ho; w = Wo;
                x = y;
                skips.push_back(x);
            }
        }
        // 4. mid (:452-457)
        {
            const int mid = m.boc.back();
            T y = resblock("mid_block.resnets.0", x, mid, mid, nullptr);      // x = the last skip: stays
            T z = transformer("mid_block.attentions.0", y, mid, m.heads.back());
            drop(y);
            x = resblock("mid_block.resnets.1", z, mid, mid, nullptr);
            drop(z);
        }
        // 5. up (:460-478): the skip is read in place (norm1 and the shortcut projection take two sources)
        for (auto& bp : m.up) {
            const std::string bpre = "up_blocks." + std::to_string(bp.idx);
            for (size_t j = 0; j < bp.layers.size(); ++j) {
                T sk = skips.back();
                skips.pop_back();
                T y = resblock(bpre + ".resnets." + std::to_string(j), x, bp.layers[j].first, bp.layers[j].second, &sk);
                drop(x);
                drop(sk);
                if (bp.attn) { T z = transformer(bpre + ".attentions." + std::to_string(j), y, bp.layers[j].second, bp.heads); drop(y); y = z; }
                x = y;
            }
            if (bp.resample) {
                int Ho, Wo;
                T y = conv3x3_up4(x, B * F, h, w, bp.ch, bpre + ".upsamplers.0.conv.weight", bpre + ".upsamplers.0.conv.bias", &Ho, &Wo);
                drop(x);
                h = Ho; w = Wo;
                x = y;
            }
        }
        // 6. out (:481-486)
        T gn = groupnorm(x, "conv_norm_out", B * F, 1e-5f, true);
        drop(x);
        T y = conv3x3(gn, B * F, h, w, c0, "conv_out.weight", "conv_out.bias", 1, false, Epi(), nullptr, nullptr, false);
        drop(gn);
        launch1d(k_nhwc_to_nchw, (long long)B * F * m.out_ch * h * w, y.p, out, B * F, m.out_ch, h * w, y.cols);
        drop(y);
        for (auto& kv : cross) drop(kv.second);
        cross.clear();
        drop(temb_all);
    }
};

int check_shape(const syn3r_unet* m, int B, int F, int h, int w, int ehs_rows, int ctx_group) {
    SYN3R_REQUIRE(unet_live(m), "unet: not a live handle (syn3r_unet_create)");
    SYN3R_REQUIRE(B > 0 && B <= 64 && F > 0 && F <= 32 && SYN3R_SIDE_OK(h) && SYN3R_SIDE_OK(w), "unet: bad sizes B=%d F=%d h=%d w=%d (F <= 32)", B, F, h, w);
    SYN3R_REQUIRE((long long)B * F * h * w <= SYN3R_DIM_MAX, "unet: B*F*h*w = %lld rows is beyond the operators' limit", (long long)B * F * h * w);
    const int down = 1 << (m->boc.size() - 1);
    SYN3R_REQUIRE(h % down == 0 && w % down == 0, "unet: h and w must be multiples of %d", down);
    SYN3R_REQUIRE(ehs_rows == 1 || ehs_rows == B, "unet: encoder_hidden_states must have 1 (shared) or B rows, got %d", ehs_rows);
    SYN3R_REQUIRE(ctx_group >= 0 && (ctx_group == 0 || B % ctx_group == 0), "unet: ctx_group=%d must divide the batch size %d", ctx_group, B);
    return SYN3R_OK;
}

}  // namespace

extern "C" size_t syn3r_unet_workspace_bytes(syn3r_unet* m, int B, int F, int h, int w, int ehs_rows) {
    if (check_shape(m, B, F, h, w, ehs_rows, 0)) return 0;
    try {
    Run r(*m, B, F, h, w, 1, ehs_rows);
    r.dry = true;
    r.ar.reset((char*)4096, (size_t)1 << 46);
    r.forward(nullptr, 0.0, (const __half*)4096, r.shared_ctx ? 1 : B, nullptr, nullptr);
    return r.ok() ? r.ar.peak + 256 : 0;
    } catch (...) { set_error("unet_workspace_bytes: unexpected exception"); return 0; }
}

extern "C" int syn3r_unet_forward(syn3r_unet* m, const void* sample, double timestep, const void* encoder_hidden_states, int ehs_rows,
                                  const float* added_time_ids, void* out, int B, int F, int h, int w, int ctx_group, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    int rc = check_shape(m, B, F, h, w, ehs_rows, ctx_group);
    if (rc) return rc;
    SYN3R_REQUIRE(sample && encoder_hidden_states && added_time_ids && out, "unet_forward: null tensor");
    SYN3R_REQUIRE(workspace && ((uintptr_t)workspace % 256) == 0, "unet_forward: workspace must be non-null and 256-byte aligned");
    SYN3R_REQUIRE((((uintptr_t)sample | (uintptr_t)encoder_hidden_states | (uintptr_t)out) % 16) == 0, "unet_forward: misaligned tensor");
    try {
    Run r(*m, B, F, h, w, ctx_group > 0 ? ctx_group : B, ehs_rows);
    r.ar.reset((char*)workspace, workspace_bytes / 256 * 256);
    r.stream = (hipStream_t)stream;
    r.forward((const __half*)sample, timestep, (const __half*)encoder_hidden_states, r.shared_ctx ? 1 : B, added_time_ids, (__half*)out);
    if (r.ok()) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return check_hip(e, "unet_forward launch");
    }
    return r.rc;
    } catch (const std::exception& e) { set_error("unet_forward: %s", e.what()); return SYN3R_E_INVALID;
    } catch (...) { set_error("unet_forward: unexpected exception"); return SYN3R_E_INVALID; }
}
