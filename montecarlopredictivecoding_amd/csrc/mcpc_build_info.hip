// libmcpc.so, what this binary is (mcpc_build.h).  Host code only, and the ONE translation unit the Makefile compiles with the
// provenance defines (the hash of the sources, the commit, the compile line's flags): it is recompiled whenever any source of the
// library changes, so the hash it reports is always the tree's, and it costs about a second.
#include <cstdio>
#include <cstring>

#include "../../include/mcpc.h"
#include "mcpc_build.h"

extern "C" {

int mcpc_abi_version(void) { return MCPC_ABI_VERSION; }

const char* mcpc_build_info(void) {
    // exp: the umbrella of mcpc_build.h, and -- should a switch ever be added without being listed there -- any -DMCPC_EXP / MCPC_HEB_EXP
    // in the flags the Makefile recorded
    static const bool exp = MCPC_TIMING_BUILD != 0 || std::strstr(MCPC_BUILD_FLAGS, "MCPC_EXP") != nullptr ||
                            std::strstr(MCPC_BUILD_FLAGS, "MCPC_HEB_EXP") != nullptr;
    static char buf[1024];
    static const int n = std::snprintf(buf, sizeof buf, "libmcpc abi=%d arch=gfx950 csrc=%s commit=%s exp=%d stamps=%d flags=[%s]",
                                       MCPC_ABI_VERSION, MCPC_BUILD_CSRC_SHA, MCPC_BUILD_COMMIT, exp ? 1 : 0, MCPC_STAMPS_BUILD, MCPC_BUILD_FLAGS);
    (void)n;
    return buf;
}

}  // extern "C"
