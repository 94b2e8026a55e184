// abi.hip — error reporting for libhulc2_amd.so (see include/hulc2_amd.h for the conventions).
#include "hulc_abi_internal.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static thread_local char g_err[512] = "";

int hulc_fail(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int hulc_check_launch(const char* where) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(g_err, sizeof(g_err), "%s: launch failed: %s", where, hipGetErrorString(e));
    return -100;
}

extern "C" const char* hulc_last_error(void) { return g_err; }

// which kernel served this thread's last conv call, and the plan its launcher computed ("" after a refused call): a sibling of g_err
static thread_local char g_conv_path[256] = "";

void hulc_conv_path_clear(void) { g_conv_path[0] = 0; }
void hulc_conv_path_set(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_conv_path, sizeof(g_conv_path), fmt, ap);
    va_end(ap);
}
void hulc_conv_path_append(const char* suffix) {
    const size_t n = strlen(g_conv_path);
    snprintf(g_conv_path + n, sizeof(g_conv_path) - n, "%s", suffix);
}

extern "C" const char* hulc_conv_last_path(void) { return g_conv_path; }
extern "C" int hulc_abi_version(void) { return 7; }

// (ABI 6) A brand-new non-blocking stream of the current device (never one a graph capture has used before: see include/hulc2_amd.h).
extern "C" int hulc_stream_create(void** out) {
    if (!out) return hulc_fail(-1, "hulc_stream_create: null pointer");
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { *out = nullptr; return hulc_fail(-100, "hulc_stream_create: hipStreamCreateWithFlags failed"); }
    *out = (void*)s;
    return 0;
}
