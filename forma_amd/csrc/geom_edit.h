// geom_edit.h — edits of the layer table that travel with the next frame (forma_hip_update_geoms / _update_geoms_xf): the
// record a frame slot's staging block is made of and the launch that applies a block to the slot's table (geom_edit.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/forma_hip.h"

// 48 bytes, 16-byte aligned: three uint4 loads.  An ENTRY record replaces table[first] by `entry`; a RANGE record gives
// table[first .. first + count) entry.xf and bit FORMA_GEOM_HAS_XF of entry.flags — `order` and the other flag bits stay.
constexpr uint32_t GE_ENTRY = 0u, GE_RANGE = 1u;
struct alignas(16) GeomEditRec {
    uint32_t kind, first, count, pad;
    forma_geom_t entry;
};
static_assert(sizeof(GeomEditRec) == 48 && sizeof(forma_geom_t) == 32, "record layout");

constexpr uint32_t GE_THREADS = 256, GE_MAX_BLOCKS = 1024;
// One launch: recs[0 .. n_range) are RANGE records, recs[n_range .. n_range + n_entry) ENTRY records.  The caller hands a launch
// records that touch pairwise disjoint slots (a slot that several pending edits name is split over launches, in order);
// slots at or beyond n_geoms are skipped.  `table` is 32-byte strided in a 256-byte-aligned allocation.
void launch_geom_edit(hipStream_t s, const GeomEditRec* recs, uint32_t n_range, uint32_t n_entry, uint32_t max_range_count,
                      forma_geom_t* table, uint32_t n_geoms);
