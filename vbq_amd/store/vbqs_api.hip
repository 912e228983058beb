// libvbq_store.so: the library's own error string and ABI version (vbq_store.h).  The sources of this directory share the
// headers of vbq_amd/csrc but are built with hidden visibility: vbq::set_error below is this library's own, and no C++ symbol
// of any of the libraries is visible to another.  gfx950 / ROCm only.
#include <stdarg.h>
#include <stdio.h>

#include "vbq_common.h"
#include "vbq_store.h"

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
}  // namespace vbq

#pragma GCC visibility push(default)
extern "C" int vbqs_abi_version(void) { return VBQS_ABI_VERSION; }

extern "C" const char *vbqs_last_error(void) { return vbq::g_err; }
#pragma GCC visibility pop
