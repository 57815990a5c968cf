// stroke.h — stroke expansion on the device (forma_hip_geometry_append_stroked): the argument record of the three kernels in
// stroke.hip and their launches.  A stroke is a map from the flattened points of one append to more points of the same kind:
// closed polygonal pieces (bodies, joins, caps), all wound the same way, whose union under FillRule::NonZero is the stroke.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/forma_hip.h"

constexpr uint32_t SK_THREADS = 256;
// a half width beyond this is FORMA_E_ARG: wider than the widest canvas, and it bounds a round fan at 1140 steps
constexpr float SK_MAX_HALF_WIDTH = 65536.0f;

struct StrokeArgs {
    // the points of the append as k_flatten_store wrote them (affines applied), and their line slots
    const float* sx; const float* sy; const uint32_t* sslot;
    uint32_t n_src;
    // stroked contours, ascending: 3 words each — first point, last point (inclusive; it carries FORMA_NONE), style index
    const uint32_t* contours; uint32_t n_contours;
    // 4 words per stroke range: half_width, miter_limit (f32 bits), join, cap
    const uint32_t* styles;
    uint32_t* counts;                // [n_src] output points of each source point
    uint32_t* block_base;            // [blocks] k_stroke_count: sum of a workgroup's counts; k_stroke_scan: exclusive prefix
    unsigned long long* total;       // all output points
    // the store
    uint32_t base, limit;            // first output point, end of the store after the append (no thread writes at or beyond it)
    float* x; float* y; uint32_t* slot;
};

inline uint32_t stroke_blocks(uint32_t n_src) { return (n_src + SK_THREADS - 1) / SK_THREADS; }
// counts and the workgroups' sums, then their exclusive scan and the total: the host reads *total to size the store
void launch_stroke_count(hipStream_t s, const StrokeArgs& A);
// the pieces, written at store + base + offset
void launch_stroke_emit(hipStream_t s, const StrokeArgs& A);
