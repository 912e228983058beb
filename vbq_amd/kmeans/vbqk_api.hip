// libvbq_kmeans.so: the library's own error string, compute-unit count and ABI version (include/vbq_kmeans.h).  The sources of
// this directory share the headers of vbq_amd/csrc but are built with hidden visibility: vbq::set_error and vbq::num_cus
// below are this library's own, and no C++ symbol of any of the libraries is visible to another.  gfx950 / ROCm only.
#include <stdarg.h>
#include <stdio.h>

#include "vbq_common.h"
#include "vbq_kmeans.h"

namespace vbq {
namespace {
thread_local char g_err[512] = "";
}
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
// hipDeviceProp_t::multiProcessorCount of the current device, cached per device (vbq_common.h)
int num_cus() {
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        dev = 0;
    }
    if (cached[dev] <= 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            n = 256;                                             // MI355X; only reached when the query itself fails
        }
        cached[dev] = n;
    }
    return cached[dev];
}
}  // namespace vbq

#pragma GCC visibility push(default)
extern "C" int vbqk_abi_version(void) { return VBQK_ABI_VERSION; }

extern "C" const char *vbqk_last_error(void) { return vbq::g_err; }
#pragma GCC visibility pop
