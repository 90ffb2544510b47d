// vibo_host.hpp -- the host-side facts that the planner (vibo_planner.hip), the dispatch (vibo_capi.hip) and the extern "C" tails of
// the other units share, each stated once: the calling thread's error string and the one failed-launch path, the compute-unit count,
// 256-byte rounding, the workspace check, the panel split of the item axis and the launch shape of the conditional passes.
// Host-only: nothing here is device code, and nothing keeps state but the error string.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace vibo {

// the calling thread's last error (vibo_last_error_string); fail() formats it and returns `code` (vibo_planner.hip)
int fail(int code, const char* fmt, ...);
const char* last_error();

// A failed launch or runtime call: the positive HIP code, with `what` and the runtime's own words as the thread's error string.
inline int hip_fail(hipError_t e, const char* what) {
    return fail((int)e > 0 ? (int)e : 999, "%s: %s", what, hipGetErrorString(e));
}
inline int hip_rc(hipError_t e, const char* what) { return e == hipSuccess ? 0 : hip_fail(e, what); }
// ... of the launch just made: 0, or hip_fail of hipGetLastError()
inline int launch_rc(const char* what) { return hip_rc(hipGetLastError(), what); }

// compute units of the current device (asked per call: the library keeps no state between calls)
inline int device_cus() {
    int dev = 0, n = 0;
    return (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
}
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// a caller's workspace against the bytes its plan asks for: 0, or -7 (error string set)
inline int check_workspace(const void* workspace, size_t have, size_t need) {
    if (!workspace || have < need) return fail(-7, "workspace too small: %zu < %zu", have, need);
    if ((uintptr_t)workspace & 255) return fail(-7, "workspace must be 256-byte aligned");
    return 0;
}

// Panels: a row-split launch takes up to kPanelItems items; panel pn of a row of I items covers [pn * kPanelItems, ... + items)
constexpr int kPanelItems = 1024;
inline int panel_count(int I) { return (I + kPanelItems - 1) / kPanelItems; }
struct PanelSpan { int item0, items; };
inline PanelSpan panel_span(int I, int pn) {
    const int item0 = pn * kPanelItems;
    return {item0, I - item0 < kPanelItems ? I - item0 : kPanelItems};
}

// cond_pre / cond_post (vibo_cond.hip) take 4 ability dims per launch: their own template width (3PL widens the split kernel's) and
// the waves per workgroup over `items` items
struct CondPassShape { int at, waves; };
inline CondPassShape cond_pass_shape(int A, int items) { return {A == 1 ? 1 : A <= 2 ? 2 : 4, (items + 255) / 256}; }

}  // namespace vibo
