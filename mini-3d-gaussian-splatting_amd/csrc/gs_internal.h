// gs_internal.h -- shared by the library's .hip files; not part of the C ABI.
#pragma once
#include "gsplat_mi355x.h"

// set gs_last_error() (fmt has one %s, filled with `what`) and return s
__attribute__((visibility("hidden"))) gs_status gs_internal_fail(gs_status s, const char *fmt, const char *what);
// GS_ERR_LAUNCH with the HIP error text if the last launch failed, else GS_OK
__attribute__((visibility("hidden"))) gs_status gs_internal_check_launch(const char *what);

// gs_radix_sort_pairs; n_dev (optional): a device word, the items are
// min(*n_dev, n) and n sizes the launches (a device-resident frame's tile sort)
__attribute__((visibility("hidden"))) gs_status gs_internal_radix_sort_pairs(
    uint32_t *keys, uint32_t *vals, uint32_t *keys_alt, uint32_t *vals_alt, int32_t n, int32_t begin_bit,
    int32_t end_bit, int32_t vals_are_iota, void *workspace, size_t workspace_bytes, int32_t *result_in_alt,
    const uint32_t *n_dev, gs_stream_t stream);
// Behind a device-resident frame's blend: when gs_bin_count flagged the frame
// (counters[4] != 0), image / alpha / depth become those of a frame that
// draws nothing -- the background once, zeros (renderer.py:74-83).
__attribute__((visibility("hidden"))) gs_status gs_internal_failed_frame_pixels(const uint32_t *counters,
                                                                               const gs_camera *cam, float *image,
                                                                               float *alpha, float *depth,
                                                                               gs_stream_t stream);
// A stable sort of n <= gs_internal_small_sort_max() (key, value) pairs by the
// keys' low `bits` bits in one workgroup (LDS passes): keys / vals in
// (vals NULL: the input positions), keys_out / vals_out out -- the result of
// gs_radix_sort_pairs over bits [0, bits) in one launch.
__attribute__((visibility("hidden"))) int32_t gs_internal_small_sort_max(void);
__attribute__((visibility("hidden"))) gs_status gs_internal_small_sort(const uint32_t *keys, const uint32_t *vals,
                                                                      uint32_t *keys_out, uint32_t *vals_out,
                                                                      int32_t n, int32_t bits, const uint32_t *n_dev,
                                                                      gs_stream_t stream);
