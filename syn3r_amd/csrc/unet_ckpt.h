// The UNet's checkpoint reader (unet_ckpt.hip): a diffusers directory in, the block plan and every weight in its kernel layout
// out.  Host-only: no HIP type on this interface, so the reader builds and runs without a device (tests/unet_ckpt_driver.cpp).
#pragma once
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace syn3r {

typedef unsigned short u16;                                             // fp16 bits on the host

struct BlockPlan { int idx; bool attn; std::vector<std::pair<int, int>> layers; bool resample; int ch, heads; };
struct HostPack { std::string name; long long rows, cols; std::vector<u16> d; };     // a packed tensor ([rows, cols], cols = the rest)

struct Checkpoint {                                                     // everything unet_create needs before its first device call
    int in_ch = 8, out_ch = 4, add_dim = 256, proj_in = 768;
    std::vector<int> boc, heads, layers, cross;
    std::vector<BlockPlan> down, up;
    std::vector<HostPack> packs;                                        // in the order of the device blob: it fixes the blob layout
    std::unordered_map<std::string, std::pair<double, double>> alpha;   // mix_factor -> (alpha, 1 - alpha) as the fp16 values the reference uses
    std::unordered_map<std::string, std::pair<int, int>> temb_slice;    // time_emb_proj name -> its rows of time_emb_proj.all
    std::vector<std::string> temb_names;
};

// Reads <weights_dir>/config.json and diffusion_pytorch_model[.<variant>].safetensors.  SYN3R_OK, or set_error + a status.
// It parses files the library does not control and may throw what the standard library throws (bad_alloc): the caller
// catches at the extern "C" boundary.
int load_checkpoint(const char* weights_dir, const char* variant, Checkpoint& out);

}  // namespace syn3r
