// hulc_abi_internal.h — error plumbing shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/hulc2_amd.h"

int hulc_fail(int code, const char* msg);          // records msg for hulc_last_error(), returns code
int hulc_check_launch(const char* where);          // hipGetLastError() -> 0 / -100

// hulc_conv_last_path(): the report of which kernel served the last conv call of this thread, written by the launchers once a launch is
// issued.  Output only: no launcher, kernel or dispatch condition reads it.
void hulc_conv_path_clear(void);
void hulc_conv_path_set(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void hulc_conv_path_append(const char* suffix);

// wgrad_taps.hip: the conv_taps_wp items of hulc_wgrad_group that run as nine-tap tiles (one pass over the operands)
int hulc_wgrad_taps_takes(const hulc_wgrad_item* d);
long hulc_wgrad_taps_workspace(const hulc_wgrad_item* const* items, int n);       // slab bytes
int hulc_wgrad_taps_launch(const hulc_wgrad_item* const* items, int n, void* slabs, hipStream_t s);

// gemm_tn128.hip / gemm_nt128.hip, tried first by hulc_gemm (gemm.hip): 1 = the shape was taken, 0 = the generic kernel must run, < 0 = error
int hulc_gemm_tn128_try(const hulc_gemm_desc* d, hipStream_t s);
int hulc_gemm_nt128_try(const hulc_gemm_desc* d, hipStream_t s);
