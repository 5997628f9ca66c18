// Stand-alone driver of the UNet's checkpoint reader (syn3r_amd/csrc/unet_ckpt.hip) for tests/test_unet_ckpt_cpu.py: the reader
// alone, no HIP, built with AddressSanitizer and UBSan.
//   usage: unet_ckpt_driver <dir> <variant or -> [dump-file]
// Failure: the reader's error message on stdout, exit 1.  Success: exit 0, and with a dump file everything the reader produced,
// as flat little-endian records (str = u32 length + bytes):
//   u32 count, then per pack   str name, i64 rows, i64 cols, u64 n, n x u16 (the fp16 bits)   - in the reader's order
//   u32 count, then per alpha  str name, f64 alpha, f64 one_minus_alpha
//   u32 count, then per slice  str name, i32 begin, i32 end                                    - rows of time_emb_proj.all
#include "../syn3r_amd/csrc/unet_ckpt.h"
#include "../include/syn3r_hip.h"
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <exception>

static char g_error[4096];
namespace syn3r {
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace syn3r

template <class V> static void put(FILE* f, V v) { fwrite(&v, sizeof v, 1, f); }
static void put_str(FILE* f, const std::string& s) { put(f, (uint32_t)s.size()); fwrite(s.data(), 1, s.size(), f); }

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s <dir> <variant or -> [dump-file]\n", argv[0]); return 2; }
    syn3r::Checkpoint ck;
    int rc = SYN3R_E_INVALID;
    try {                                                       // what syn3r_unet_create does around the reader
        rc = syn3r::load_checkpoint(argv[1], strcmp(argv[2], "-") ? argv[2] : nullptr, ck);
    } catch (const std::exception& e) {
        syn3r::set_error("unet_create: %s", e.what());
    } catch (...) {
        syn3r::set_error("unet_create: unexpected exception");
    }
    if (rc != SYN3R_OK) { printf("%s\n", g_error); return 1; }
    if (argc > 3) {
        FILE* f = fopen(argv[3], "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
        put(f, (uint32_t)ck.packs.size());
        for (auto& p : ck.packs) {
            put_str(f, p.name); put(f, (int64_t)p.rows); put(f, (int64_t)p.cols); put(f, (uint64_t)p.d.size());
            fwrite(p.d.data(), 2, p.d.size(), f);
        }
        put(f, (uint32_t)ck.alpha.size());
        for (auto& kv : ck.alpha) { put_str(f, kv.first); put(f, kv.second.first); put(f, kv.second.second); }
        put(f, (uint32_t)ck.temb_slice.size());
        for (auto& kv : ck.temb_slice) { put_str(f, kv.first); put(f, (int32_t)kv.second.first); put(f, (int32_t)kv.second.second); }
        if (fclose(f)) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    }
    return 0;
}
