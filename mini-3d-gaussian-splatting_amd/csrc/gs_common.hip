// gs_common.hip -- what every stage file reports through: the library's one
// thread-local error string (gs_last_error), its two writers declared in
// gs_internal.h, and the ABI version.  No kernel lives here.
//
// The render path's stages, one file each (each cites the reference lines it
// replaces): gs_project.hip, gs_sort.hip, gs_bin.hip, gs_blend.hip; the
// training kernels: gs_adam.hip, gs_loss.hip, gs_densify.hip; the whole-frame
// entry points over them: gs_render.hip.  Layout and roofline notes: DESIGN.md.
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "gs_internal.h"

namespace {
thread_local char g_err[512];
}  // namespace

gs_status gs_internal_fail(gs_status s, const char *fmt, const char *what) {
  snprintf(g_err, sizeof(g_err), fmt, what);
  return s;
}

gs_status gs_internal_check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: launch failed: %s", what, hipGetErrorString(e));
    return GS_ERR_LAUNCH;
  }
  return GS_OK;
}

// ============================================================ C ABI =======
extern "C" {

int32_t gs_abi_version(void) { return GS_ABI_VERSION; }

const char *gs_last_error(void) { return g_err; }

}  // extern "C"
