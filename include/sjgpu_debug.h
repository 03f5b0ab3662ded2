/* include/sjgpu_debug.h -- C-ABI of libsjgpu.so, diagnostics of the single-pass workspace: what lies on the device between two calls, and how often a
 * call gave up.  The single-pass kernels (sjgpu_set_pipeline: SJGPU_PIPELINE_FUSED, and AUTO on small inputs) clear nothing in front of themselves: each
 * trusts that the kernel before it left the context's [tile descriptors][control words] all zero.  These two calls let a test look.
 * An extension of include/sjgpu.h (the context and sjgpu_scan_result are declared there); a header of its own so that programs built against the other
 * headers are not rebuilt for it. */
#ifndef SJGPU_DEBUG_H
#define SJGPU_DEBUG_H

#include "sjgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The context's single-pass workspace as it lies on the device, and the device's copy of the last result.  *words_out = the words allocated
 * (tile descriptors + control words; 0: no workspace yet), of which up to cap_words are copied to words_host.  Synchronous and without a stream
 * argument, like sjgpu_debug_trace_stage1: waits for the device, then plain copies, no kernel.  Allocates nothing and changes nothing about what the
 * next call does. */
int sjgpu_debug_read_workspace(sjgpu_ctx *ctx, sjgpu_scan_result *result_out, uint64_t *words_host, size_t cap_words, size_t *words_out);

/* How many results carrying SJGPU_F_INTERNAL this context has read since it was created (or taken back from the pool): each is a single-pass call
 * that gave up -- which the host-buffer entry points re-run on the split pipeline without a word. */
uint64_t sjgpu_debug_gave_up_count(const sjgpu_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
