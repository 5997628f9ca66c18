// The checkpoint reader behind syn3r_unet_create: config.json and the safetensors file of a diffusers directory
// (`from_pretrained(<local dir>, torch_dtype=float16, variant="fp16")`, model/diffusionGS.py:1089) into the block plan and the
// kernel-side weight layouts that syn3r_amd/unet/model.py:_declare / _pack build in Python (OHWI convolutions, fused qkv, GEGLU
// row groups, stacked time-embedding projections).  Host code only: it parses files the library does not control and never
// touches the device, so it includes no HIP and also compiles as plain C++17 (`-x c++`) - which is how
// tests/test_unet_ckpt_cpu.py runs it under AddressSanitizer / UBSan on hostile headers and compares every pack with the Python twin.
#include "unet_ckpt.h"
#include "error.h"
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ctype.h>
#include <algorithm>
#include <map>

using namespace syn3r;

namespace {

// ------------------------------------------------------------------------------------------------ JSON (config.json, safetensors header)
struct JVal {
    enum Type { NUL, NUM, STR, ARR, OBJ, BOOL } type = NUL;
    double num = 0;
    std::string str;
    std::vector<JVal> arr;
    std::vector<std::pair<std::string, JVal>> obj;
    const JVal* get(const char* k) const {
        for (auto& kv : obj) if (kv.first == k) return &kv.second;
        return nullptr;
    }
};
struct JParser {
    const char* p; const char* e; bool ok = true;
    void ws() { while (p < e && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) ++p; }
    bool lit(const char* s) { size_t n = strlen(s); if ((size_t)(e - p) >= n && !memcmp(p, s, n)) { p += n; return true; } return false; }
    std::string string_() {
        std::string s;
        if (p >= e || *p != '"') { ok = false; return s; }
        ++p;
        while (p < e && *p != '"') {
            if (*p == '\\' && p + 1 < e) {
                ++p;
                switch (*p) {
                    case 'n': s += '\n'; break;
                    case 't': s += '\t'; break;
                    case 'u':                                  // \uXXXX: not needed for tensor names; the four digits must exist
                        if (e - p < 5) { ok = false; return s; }
                        s += '?'; p += 4; break;
                    default: s += *p;
                }
                ++p;
            } else s += *p++;
        }
        if (p >= e) { ok = false; return s; }
        ++p;
        return s;
    }
    JVal value(int depth = 0) {
        JVal v;
        ws();
        if (p >= e || depth > 64) { ok = false; return v; }
        if (*p == '{') {
            v.type = JVal::OBJ; ++p; ws();
            if (p < e && *p == '}') { ++p; return v; }
            while (ok) {
                ws();
                std::string k = string_();
                ws();
                if (p >= e || *p != ':') { ok = false; break; }
                ++p;
                v.obj.emplace_back(std::move(k), value(depth + 1));
                ws();
                if (p < e && *p == ',') { ++p; continue; }
                if (p < e && *p == '}') { ++p; break; }
                ok = false;
            }
        } else if (*p == '[') {
            v.type = JVal::ARR; ++p; ws();
            if (p < e && *p == ']') { ++p; return v; }
            while (ok) {
                v.arr.push_back(value(depth + 1));
                ws();
                if (p < e && *p == ',') { ++p; continue; }
                if (p < e && *p == ']') { ++p; break; }
                ok = false;
            }
        } else if (*p == '"') { v.type = JVal::STR; v.str = string_(); }
        else if (lit("true")) { v.type = JVal::BOOL; v.num = 1; }
        else if (lit("false")) { v.type = JVal::BOOL; v.num = 0; }
        else if (lit("null")) { v.type = JVal::NUL; }
        else {
            // the header is a slice of an mmap'd file: not NUL-terminated, so the number is parsed from a bounded copy
            char buf[64];
            size_t n = 0;
            while (p + n < e && n < sizeof(buf) - 1 && (isdigit((unsigned char)p[n]) || p[n] == '-' || p[n] == '+' || p[n] == '.' || p[n] == 'e' || p[n] == 'E')) ++n;
            memcpy(buf, p, n);
            buf[n] = 0;
            char* end = nullptr;
            v.type = JVal::NUM; v.num = n ? strtod(buf, &end) : 0.0;
            if (n == 0 || end != buf + n || !(v.num == v.num)) ok = false; else p += n;
        }
        return v;
    }
};

bool read_file(const std::string& path, std::string& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
    fclose(f);
    return true;
}

// ------------------------------------------------------------------------------------------------ safetensors
struct StEntry { std::string dtype; std::vector<long long> shape; size_t begin = 0, end = 0; };
struct StFile {
    int fd = -1; const unsigned char* map = nullptr; size_t size = 0, data0 = 0;
    std::unordered_map<std::string, StEntry> entries;
    ~StFile() { if (map) munmap((void*)map, size); if (fd >= 0) close(fd); }
    bool open_(const std::string& path, std::string& err) {
        fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) { err = "cannot open " + path; return false; }
        struct stat sb;
        if (fstat(fd, &sb) || sb.st_size < 8) { err = path + ": not a safetensors file"; return false; }
        size = (size_t)sb.st_size;
        map = (const unsigned char*)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (map == MAP_FAILED) { map = nullptr; err = "mmap failed on " + path; return false; }
        unsigned long long hl = 0;
        memcpy(&hl, map, 8);
        if (hl == 0 || hl > size - 8) { err = path + ": bad header length"; return false; }
        data0 = 8 + (size_t)hl;
        JParser jp{(const char*)map + 8, (const char*)map + 8 + hl};
        JVal h = jp.value();
        if (!jp.ok || h.type != JVal::OBJ) { err = path + ": header is not JSON"; return false; }
        for (auto& kv : h.obj) {
            if (kv.first == "__metadata__") continue;
            const JVal *dt = kv.second.get("dtype"), *sh = kv.second.get("shape"), *off = kv.second.get("data_offsets");
            if (!dt || !sh || !off || off->arr.size() != 2) { err = path + ": malformed entry " + kv.first; return false; }
            StEntry en;
            en.dtype = dt->str;
            // dimensions and offsets are file contents: integers in [0, 2^53) only, the element count bounded by the file size
            auto whole = [](const JVal& x) { return x.type == JVal::NUM && x.num >= 0 && x.num < 9007199254740992.0 && x.num == (double)(unsigned long long)x.num; };
            if (sh->type != JVal::ARR || sh->arr.size() > 8 || !whole(off->arr[0]) || !whole(off->arr[1])) { err = path + ": malformed entry " + kv.first; return false; }
            unsigned long long count = 1;
            for (auto& d : sh->arr) {
                if (!whole(d)) { err = path + ": bad shape in entry " + kv.first; return false; }
                if (__builtin_mul_overflow(count, (unsigned long long)d.num, &count) || count > (unsigned long long)size) { err = path + ": shape of entry " + kv.first + " exceeds the file"; return false; }
                en.shape.push_back((long long)d.num);
            }
            en.begin = (size_t)off->arr[0].num; en.end = (size_t)off->arr[1].num;
            if (en.end < en.begin || en.end > size - data0) { err = path + ": entry " + kv.first + " outside the file"; return false; }
            entries.emplace(kv.first, std::move(en));
        }
        return true;
    }
};

inline u16 f32_to_f16_bits(float f) { _Float16 h = (_Float16)f; u16 b; memcpy(&b, &h, 2); return b; }
inline float f16_bits_to_f32(u16 b) { _Float16 h; memcpy(&h, &b, 2); return (float)h; }

// a checkpoint tensor as fp16 bits on the host (F16 as stored; F32 / BF16 rounded once, as `.to(torch.float16)` does)
bool host_f16(const StFile& f, const StEntry& e, std::vector<u16>& out, std::string& err) {
    unsigned long long cnt = 1;
    for (long long d : e.shape)
        if (d < 0 || __builtin_mul_overflow(cnt, (unsigned long long)d, &cnt)) { err = "bad shape"; return false; }
    const bool f32 = e.dtype == "F32", bf16 = e.dtype == "BF16";
    if (!f32 && !bf16 && e.dtype != "F16") { err = "unsupported dtype " + e.dtype; return false; }
    const size_t esz = f32 ? 4 : 2;
    if (cnt > (e.end - e.begin) / esz || cnt * esz != e.end - e.begin) { err = "size mismatch"; return false; }   // before any allocation
    const size_t n = (size_t)cnt;
    const unsigned char* src = f.map + f.data0 + e.begin;
    out.resize(n);
    if (f32) {
        for (size_t i = 0; i < n; ++i) { float v; memcpy(&v, src + 4 * i, 4); out[i] = f32_to_f16_bits(v); }
    } else if (bf16) {
        for (size_t i = 0; i < n; ++i) { u16 b; memcpy(&b, src + 2 * i, 2); const unsigned int u = (unsigned)b << 16; float v; memcpy(&v, &u, 4); out[i] = f32_to_f16_bits(v); }
    } else if (n) {
        memcpy(out.data(), src, n * 2);
    }
    return true;
}

// ------------------------------------------------------------------------------------------------ model
int fail(const char* fmt, const std::string& a) { set_error(fmt, a.c_str()); return SYN3R_E_INVALID; }

std::vector<int> int_list(const JVal* v, size_t n, int dflt) {
    std::vector<int> r;
    if (!v) return std::vector<int>(n, dflt);
    if (v->type == JVal::ARR) { for (auto& x : v->arr) r.push_back((int)x.num); }
    else r.assign(n, (int)v->num);
    return r;
}

// model.py:_declare - the block plan of unet_spatio_temporal_condition.py:140-330
int build_plan(Checkpoint& m, const JVal& cfg) {
    auto num = [&](const char* k, int d) { const JVal* v = cfg.get(k); return v && v->type == JVal::NUM ? (int)v->num : d; };
    m.in_ch = num("in_channels", 8); m.out_ch = num("out_channels", 4);
    m.add_dim = num("addition_time_embed_dim", 256); m.proj_in = num("projection_class_embeddings_input_dim", 768);
    const JVal* b = cfg.get("block_out_channels");
    m.boc = b ? int_list(b, 0, 0) : std::vector<int>{320, 640, 1280, 1280};
    const size_t n = m.boc.size();
    SYN3R_REQUIRE(n >= 1 && n <= 8, "unet_create: %zu levels", n);
    m.heads = cfg.get("num_attention_heads") ? int_list(cfg.get("num_attention_heads"), n, 0) : std::vector<int>{5, 10, 20, 20};
    m.layers = int_list(cfg.get("layers_per_block"), n, 2);
    m.cross = int_list(cfg.get("cross_attention_dim"), n, 1024);
    std::vector<int> tl = int_list(cfg.get("transformer_layers_per_block"), n, 1);
    SYN3R_REQUIRE(m.heads.size() == n && m.layers.size() == n && m.cross.size() == n && tl.size() == n, "unet_create: per-level lists of config.json do not match block_out_channels");
    for (size_t i = 0; i < n; ++i) {
        SYN3R_REQUIRE(tl[i] == 1, "unet_create: transformer_layers_per_block != 1 is not used by SVD");
        SYN3R_REQUIRE(m.boc[i] % 64 == 0 && m.boc[i] == 64 * m.heads[i], "unet_create: attention head dim must be 64 (level %zu: %d channels, %d heads)", i, m.boc[i], m.heads[i]);
        SYN3R_REQUIRE(m.layers[i] >= 1 && m.layers[i] <= 8, "unet_create: layers_per_block");
    }
    std::vector<std::string> dt, ut;
    if (const JVal* v = cfg.get("down_block_types")) for (auto& x : v->arr) dt.push_back(x.str);
    else { dt.assign(n, "CrossAttnDownBlockSpatioTemporal"); dt.back() = "DownBlockSpatioTemporal"; }
    if (const JVal* v = cfg.get("up_block_types")) for (auto& x : v->arr) ut.push_back(x.str);
    else { ut.assign(n, "CrossAttnUpBlockSpatioTemporal"); ut.front() = "UpBlockSpatioTemporal"; }
    SYN3R_REQUIRE(dt.size() == n && ut.size() == n, "unet_create: block type lists do not match block_out_channels");
    int out_ch = m.boc[0];
    for (size_t i = 0; i < n; ++i) {
        const int in_ch = out_ch;
        out_ch = m.boc[i];
        const bool attn = dt[i] == "CrossAttnDownBlockSpatioTemporal";
        if (!attn && dt[i] != "DownBlockSpatioTemporal") return fail("unet_create: %s does not exist", dt[i]);
        BlockPlan bp{(int)i, attn, {}, i != n - 1, out_ch, m.heads[i]};
        for (int j = 0; j < m.layers[i]; ++j) bp.layers.emplace_back(j == 0 ? in_ch : out_ch, out_ch);
        m.down.push_back(bp);
    }
    std::vector<int> rev(m.boc.rbegin(), m.boc.rend()), rev_heads(m.heads.rbegin(), m.heads.rend()), rev_layers(m.layers.rbegin(), m.layers.rend());
    out_ch = rev[0];
    for (size_t i = 0; i < n; ++i) {
        const bool attn = ut[i] == "CrossAttnUpBlockSpatioTemporal";
        if (!attn && ut[i] != "UpBlockSpatioTemporal") return fail("unet_create: %s does not exist", ut[i]);
        const int prev_out = out_ch;
        out_ch = rev[i];
        const int in_ch = rev[std::min(i + 1, n - 1)];
        const int nl = rev_layers[i] + 1;
        BlockPlan bp{(int)i, attn, {}, i != n - 1, out_ch, rev_heads[i]};
        for (int j = 0; j < nl; ++j) {
            const int res_skip = j == nl - 1 ? in_ch : out_ch, res_in = j == 0 ? prev_out : out_ch;
            bp.layers.emplace_back(res_in + res_skip, out_ch);
        }
        m.up.push_back(bp);
    }
    return SYN3R_OK;
}

// ------------------------------------------------------------------------------------------------ kernel-side layouts
// model.py:_pack, Conv2d 3x3: [O, I, 3, 3] -> OHWI, I padded to 64, O to 8
HostPack pack_conv3x3_ohwi(const std::string& name, const std::vector<u16>& t, long long O, long long I) {
    const long long IP = (I + 63) / 64 * 64, OP = (O + 7) / 8 * 8;
    HostPack hp{name, OP, 9 * IP, std::vector<u16>((size_t)(OP * 9 * IP), 0)};
    for (long long o = 0; o < O; ++o) for (long long i = 0; i < I; ++i) for (int y = 0; y < 3; ++y) for (int x = 0; x < 3; ++x)
        hp.d[(size_t)(((o * 3 + y) * 3 + x) * IP + i)] = t[(size_t)(((o * I + i) * 3 + y) * 3 + x)];
    return hp;
}
// model.py:_pack, Conv3d (3,1,1): [O, I, 3, 1, 1] -> [O, 3, I]
HostPack pack_conv3d_taps(const std::string& name, const std::vector<u16>& t, long long O, long long I) {
    HostPack hp{name, O, 3 * I, std::vector<u16>((size_t)(O * 3 * I))};
    for (long long o = 0; o < O; ++o) for (long long i = 0; i < I; ++i) for (int tt = 0; tt < 3; ++tt)
        hp.d[(size_t)((o * 3 + tt) * I + i)] = t[(size_t)((o * I + i) * 3 + tt)];
    return hp;
}
// The three GEGLU row orders of net.0.proj (wv [2 D, K], bv [2 D]: hidden rows, then gate rows) into pw / pb.
// ops.pack_geglu_chunked: per 64-wide hidden chunk 4 x [16 hidden | 16 gate]
void pack_geglu_chunked(const std::vector<u16>& wv, const std::vector<u16>& bv, long long D, long long K, HostPack& pw, HostPack& pb) {
    pw.rows = 2 * D; pw.cols = K; pw.d.resize((size_t)(2 * D * K)); pb.rows = 2 * D; pb.cols = 1; pb.d.resize((size_t)(2 * D));
    long long r = 0;
    for (long long j = 0; j < D / 64; ++j) for (int q = 0; q < 64; q += 16) for (int half = 0; half < 2; ++half) for (int i = 0; i < 16; ++i, ++r) {
        const long long src = (half ? D : 0) + 64 * j + q + i;
        memcpy(&pw.d[(size_t)(r * K)], &wv[(size_t)(src * K)], (size_t)K * 2);
        pb.d[(size_t)r] = bv[(size_t)src];
    }
}
// [tile hidden | tile gate] per `tile` output columns, the last tile zero-padded
void pack_geglu_tiles(const std::vector<u16>& wv, const std::vector<u16>& bv, long long D, long long K, long long tile, HostPack& pw, HostPack& pb) {
    const long long tiles = (D + tile - 1) / tile;
    pw.rows = tiles * 2 * tile; pw.cols = K; pw.d.assign((size_t)(pw.rows * K), 0); pb.rows = pw.rows; pb.cols = 1; pb.d.assign((size_t)pb.rows, 0);
    for (long long t = 0; t < tiles; ++t) {
        const long long n = std::min(tile, D - tile * t);
        memcpy(&pw.d[(size_t)(2 * tile * t * K)], &wv[(size_t)(tile * t * K)], (size_t)(n * K) * 2);
        memcpy(&pw.d[(size_t)((2 * tile * t + tile) * K)], &wv[(size_t)((D + tile * t) * K)], (size_t)(n * K) * 2);
        memcpy(&pb.d[(size_t)(2 * tile * t)], &bv[(size_t)(tile * t)], (size_t)n * 2);
        memcpy(&pb.d[(size_t)(2 * tile * t + tile)], &bv[(size_t)(D + tile * t)], (size_t)n * 2);
    }
}
// ops.pack_geglu: 80-column output tiles of the two-kernel feed-forward
void pack_geglu80(const std::vector<u16>& wv, const std::vector<u16>& bv, long long D, long long K, HostPack& pw, HostPack& pb) { pack_geglu_tiles(wv, bv, D, K, 80, pw, pb); }
// ops.pack_geglu64: 64-wide hidden chunks for the 256 x 256 tile (k_gemm_g256, round 6); D a multiple of 64, so no padding
void pack_geglu64(const std::vector<u16>& wv, const std::vector<u16>& bv, long long D, long long K, HostPack& pw, HostPack& pb) { pack_geglu_tiles(wv, bv, D, K, 64, pw, pb); }

// model.py:_pack - the kernel-side layouts, built on the host from the checkpoint's tensors
int pack_weights(Checkpoint& m, const StFile& f) {
    std::vector<HostPack>& packs = m.packs;
    std::string err;
    auto has_suffix = [](const std::string& s, const char* suf) { size_t n = strlen(suf); return s.size() >= n && !s.compare(s.size() - n, n, suf); };
    std::map<std::string, const StEntry*> names;                         // sorted: a deterministic blob layout
    for (auto& kv : f.entries) names[kv.first] = &kv.second;
    // load_state_dict's order is the DECLARATION order; the stacked time-embedding projection follows it.  Recreate that order.
    auto res_names = [&](const std::string& pre, std::vector<std::string>& out) {
        out.push_back(pre + ".spatial_res_block.time_emb_proj");
        out.push_back(pre + ".temporal_res_block.time_emb_proj");
    };
    for (auto& bp : m.down) for (size_t j = 0; j < bp.layers.size(); ++j) res_names("down_blocks." + std::to_string(bp.idx) + ".resnets." + std::to_string(j), m.temb_names);
    res_names("mid_block.resnets.0", m.temb_names);
    res_names("mid_block.resnets.1", m.temb_names);
    for (auto& bp : m.up) for (size_t j = 0; j < bp.layers.size(); ++j) res_names("up_blocks." + std::to_string(bp.idx) + ".resnets." + std::to_string(j), m.temb_names);

    std::unordered_map<std::string, size_t> stored;                      // name -> index in packs of a tensor kept as stored
    for (auto& kv : names) {
        const std::string& k = kv.first;
        const StEntry& e = *kv.second;
        std::vector<u16> t;
        if (!host_f16(f, e, t, err)) return fail("unet_create: %s", k + ": " + err);
        const auto& s = e.shape;
        if (has_suffix(k, ".weight") && s.size() == 4 && s[2] == 3 && s[3] == 3) {
            packs.push_back(pack_conv3x3_ohwi(k, t, s[0], s[1]));
        } else if (has_suffix(k, ".weight") && s.size() == 5 && s[2] == 3 && s[3] == 1 && s[4] == 1) {
            packs.push_back(pack_conv3d_taps(k, t, s[0], s[1]));
        } else if (has_suffix(k, "mix_factor")) {
            // AlphaBlender (resnet.py:789-802): alpha = sigmoid(mix_factor) in fp16 (`alpha.to(x_spatial.dtype)`), 1 - alpha in fp16 arithmetic
            if (t.empty()) return fail("unet_create: %s", k + ": bad shape");
            const float mf = f16_bits_to_f32(t[0]);                                      // (load_state_dict keeps every parameter in fp16)
            const _Float16 a = (_Float16)(1.0f / (1.0f + expf(-mf)));
            const _Float16 om = (_Float16)((_Float16)1.0f - a);
            m.alpha[k] = {(double)(float)a, (double)(float)om};
        } else {                                                                          // Linear / norm / bias / 1x1 shortcut: as stored ([rows, rest])
            HostPack hp; hp.name = k;
            hp.rows = s.empty() ? 1 : s[0];
            hp.cols = hp.rows ? (long long)t.size() / hp.rows : 0;
            hp.d = std::move(t);
            stored[k] = packs.size();
            packs.push_back(std::move(hp));
        }
    }
    // the second pass reads tensors the first kept as stored: already converted, found by name (the pointer holds until the next push_back)
    auto get = [&](const std::string& k) -> const HostPack* {
        auto it = stored.find(k);
        if (it == stored.end()) { err = "missing tensor " + k; return nullptr; }
        return &packs[it->second];
    };
    // a Linear's weight and bias for restacking: [rows, cols > 0] and one bias per row
    auto get_linear = [&](const std::string& pre, const HostPack*& w, const HostPack*& b) -> bool {
        if (!(w = get(pre + ".weight")) || !(b = get(pre + ".bias"))) return false;
        if (w->cols <= 0 || (long long)b->d.size() != w->rows) { err = pre + ".weight: bad shape"; return false; }
        return true;
    };
    // conv_out.bias padded to 8 outputs
    {
        auto it = stored.find("conv_out.bias");
        if (it == stored.end()) return fail("unet_create: %s", "missing tensor conv_out.bias");
        HostPack& hp = packs[it->second];
        hp.d.resize((hp.d.size() + 7) / 8 * 8, 0);
        hp.rows = (long long)hp.d.size(); hp.cols = 1;
    }
    // the upsamplers' 3x3 weights folded into four 2x2 phase filters (ops.pack_upsample4; the OHWI pack above is their source)
    for (size_t i = 0, n = packs.size(); i < n; ++i) {
        if (!has_suffix(packs[i].name, ".upsamplers.0.conv.weight")) continue;
        const long long O = packs[i].rows, I = packs[i].cols / 9;
        HostPack hp; hp.name = packs[i].name + "_up4"; hp.rows = 4 * O; hp.cols = 4 * I; hp.d.resize((size_t)(16 * O * I));
        if (syn3r_pack_upsample4_f16(packs[i].d.data(), hp.d.data(), (int)O, (int)I) != SYN3R_OK) return SYN3R_E_INVALID;
        packs.push_back(std::move(hp));
    }
    // fused qkv; GEGLU row groups; stacked time-embedding projections
    for (auto& kv : names) {
        const std::string& k = kv.first;
        if (has_suffix(k, "attn1.to_q.weight")) {
            const std::string pre = k.substr(0, k.size() - strlen("to_q.weight"));
            HostPack hp; hp.name = pre + "qkv";
            for (const char* part : {"to_q.weight", "to_k.weight", "to_v.weight"}) {
                const HostPack* t = get(pre + part);
                if (!t) return fail("unet_create: %s", err);
                if (t->cols <= 0) return fail("unet_create: %s", pre + part + ": bad shape");
                hp.d.insert(hp.d.end(), t->d.begin(), t->d.end());
                hp.cols = t->cols;
            }
            hp.rows = (long long)hp.d.size() / hp.cols;
            packs.push_back(std::move(hp));
        } else if (has_suffix(k, ".net.0.proj.weight")) {
            const std::string pre = k.substr(0, k.size() - strlen("weight"));
            const HostPack *w, *b;
            if (!get_linear(pre.substr(0, pre.size() - 1), w, b)) return fail("unet_create: %s", err);
            const long long K = w->cols, D = w->rows / 2;
            HostPack pw, pb, qw, qb;
            if (K == 320) {
                if (D % 64) return fail("unet_create: %s: hidden width must be a multiple of 64", k);
                pw.name = pre + "geglu_cw"; pb.name = pre + "geglu_cb";
                pack_geglu_chunked(w->d, b->d, D, K, pw, pb);
            } else {
                pw.name = pre + "geglu_w"; pb.name = pre + "geglu_b";
                pack_geglu80(w->d, b->d, D, K, pw, pb);
                if (D % 128 == 0) {                                                      // beside it, for the 256 x 256 tile
                    qw.name = pre + "geglu_w64"; qb.name = pre + "geglu_b64";
                    pack_geglu64(w->d, b->d, D, K, qw, qb);
                }
            }
            packs.push_back(std::move(pw)); packs.push_back(std::move(pb));
            if (!qw.name.empty()) { packs.push_back(std::move(qw)); packs.push_back(std::move(qb)); }
        }
    }
    {   // model.py:_pack - every resnet's time_emb_proj stacked in declaration order; each block reads its slice
        HostPack pw, pb; pw.name = "time_emb_proj.all.weight"; pb.name = "time_emb_proj.all.bias";
        int off = 0; long long K = 0;
        for (auto& nme : m.temb_names) {
            const HostPack *w, *b;
            if (!get_linear(nme, w, b)) return fail("unet_create: %s", err);
            K = w->cols;
            m.temb_slice[nme] = {off, off + (int)w->rows};
            off += (int)w->rows;
            pw.d.insert(pw.d.end(), w->d.begin(), w->d.end());
            pb.d.insert(pb.d.end(), b->d.begin(), b->d.end());
        }
        pw.rows = off; pw.cols = K; pb.rows = off; pb.cols = 1;
        packs.push_back(std::move(pw)); packs.push_back(std::move(pb));
    }
    return SYN3R_OK;
}

// diffusion_pytorch_model.<variant>.safetensors where it exists, else the plain name
int open_weights(const std::string& dir, const char* variant, StFile& f) {
    for (int plain = (variant && *variant) ? 0 : 1; plain < 2; ++plain) {
        std::string err;
        if (f.open_(dir + "/diffusion_pytorch_model." + (plain ? "" : std::string(variant) + ".") + "safetensors", err)) return SYN3R_OK;
        if (err.compare(0, 11, "cannot open")) return fail("unet_create: %s", err);      // the file is there and is not a checkpoint
    }
    return fail("unet_create: no safetensors weights under %s (diffusion_pytorch_model[.variant].safetensors)", dir);
}

}  // namespace

int syn3r::load_checkpoint(const char* weights_dir, const char* variant, Checkpoint& out) {
    const std::string dir(weights_dir);
    std::string cfg_text;
    if (!read_file(dir + "/config.json", cfg_text)) return fail("unet_create: cannot read %s/config.json", dir);
    JParser jp{cfg_text.data(), cfg_text.data() + cfg_text.size()};
    JVal cfg = jp.value();
    if (!jp.ok || cfg.type != JVal::OBJ) return fail("unet_create: %s/config.json is not a JSON object", dir);
    int rc = build_plan(out, cfg);
    if (rc) return rc;
    StFile f;
    rc = open_weights(dir, variant, f);
    return rc ? rc : pack_weights(out, f);
}

// The fold rule of the four-phase upsampling convolution (include/syn3r_hip.h): pure host code, the twin of ops.pack_upsample4.
// After a nearest-2x upsample the 3x3 window of an output pixel of parity (py, px) covers a 2x2 block of input pixels; filter rows
// ty fall on block row a as  py = 0: {0} | {1, 2},  py = 1: {0, 1} | {2}  (columns the same with px).  Each folded weight is the
// sum of its 1, 2 or 4 source taps in fp32, taken in ascending (ty, tx) order and rounded once to fp16 (nearest even).
extern "C" int syn3r_pack_upsample4_f16(const void* w, void* w4, int Cout, int Cin) {
    SYN3R_REQUIRE(w && w4, "pack_upsample4: null operand");
    SYN3R_REQUIRE(Cout > 0 && Cin > 0 && Cout <= (1 << 15) && Cin <= (1 << 15), "pack_upsample4: bad sizes Cout=%d Cin=%d", Cout, Cin);
    const _Float16* src = (const _Float16*)w;
    _Float16* dst = (_Float16*)w4;
    const size_t C = (size_t)Cin;
    for (int ph = 0; ph < 4; ++ph) {
        const int py = ph >> 1, px = ph & 1;
        for (int o = 0; o < Cout; ++o)
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) {
                    const int ty0 = py == 0 ? (a == 0 ? 0 : 1) : (a == 0 ? 0 : 2), ty1 = py == 0 ? (a == 0 ? 0 : 2) : (a == 0 ? 1 : 2);
                    const int tx0 = px == 0 ? (b == 0 ? 0 : 1) : (b == 0 ? 0 : 2), tx1 = px == 0 ? (b == 0 ? 0 : 2) : (b == 0 ? 1 : 2);
                    _Float16* d = dst + ((((size_t)ph * Cout + o) * 2 + a) * 2 + b) * C;
                    for (size_t c = 0; c < C; ++c) {
                        float s = 0.f;
                        bool first = true;
                        for (int ty = ty0; ty <= ty1; ++ty)
                            for (int tx = tx0; tx <= tx1; ++tx) {
                                const float v = (float)src[(((size_t)o * 3 + ty) * 3 + tx) * C + c];
                                s = first ? v : s + v;
                                first = false;
                            }
                        d[c] = (_Float16)s;
                    }
                }
    }
    return SYN3R_OK;
}
