// Error reporting of libsyn3r_hip.so without HIP: the status codes of the public header, the thread's last-error message and
// the argument check every entry starts with.  Host-only translation units (unet_ckpt.hip) include this and not common.h.
#pragma once
#include "../../include/syn3r_hip.h"

namespace syn3r {

void set_error(const char* fmt, ...);

}  // namespace syn3r

#define SYN3R_REQUIRE(cond, ...)                 \
    do {                                         \
        if (!(cond)) {                           \
            syn3r::set_error(__VA_ARGS__);       \
            return SYN3R_E_INVALID;              \
        }                                        \
    } while (0)
