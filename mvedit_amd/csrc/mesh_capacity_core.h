// Bounds arithmetic of the capacity (host-read-free) form of the MESH optimisation iteration: which vertex and face rows exist when the
// mesh tensors are sized by caller-chosen CAPACITIES (v_cap, f_cap) and the numbers of live rows are counts in device memory.  Used by
// dmtet.hip, mesh_reg.hip and raster.hip; the same source compiles for the host, where tests/test_mesh_capacity.py walks it under the
// address and undefined-behaviour sanitizers against a Python restatement of the rules below.
//
// Rules.  The extraction finds (n_verts, n_faces); the caller's buffers hold v_cap vertex rows and f_cap face rows.
//   * counts[2] = (n_verts, n_faces), the TRUE totals, also when they do not fit: the caller grows the capacity from them at a point
//     where it synchronises anyway;
//   * overflow = 1 when n_verts > v_cap or n_faces > f_cap, else 0;
//   * live[2] = (n_verts, n_faces) when nothing overflows, (0, 0) when anything does: an overflowed mesh is the EMPTY mesh, never a
//     truncated one whose faces point at vertices that were not written;
//   * a row index exists when it is below min(max(count, 0), capacity): every count-aware kernel clamps what it reads
//     (mcap_live); a null count pointer is the exact form, every row is live;
//   * rows at and beyond the live count are written on every call, never left stale:
//       vertices 0.0, faces (0, 0, 0), edges (0, 0), opposites -1, vn (0, 0, 0), face_normals (0, 0, 0).
//     The padded face is index-degenerate on purpose: its fixed-point area is zero, so the rasteriser drops it before the depth buffer,
//     and every later render kernel reaches triangles only through the ids the rasteriser wrote.  The two padded normals are what the
//     exact kernels give for such a face and for a vertex no face touches (0 / max(0, 1e-12)).
//   * a fixed-order reduction over 256-row blocks runs over the blocks that hold live rows only (mcap_blocks), in the exact call's
//     order, so its result equals the exact call on the live rows bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MVE_MCAP_FN __host__ __device__ __forceinline__
#else
#define MVE_MCAP_FN static inline
#endif

#define MVE_MCAP_PAD_VERT 0.0f     // every component of a padded vertex row
#define MVE_MCAP_PAD_INDEX 0       // every index of a padded face / edge row
#define MVE_MCAP_PAD_OPP (-1)      // every entry of a padded opposites row
#define MVE_MCAP_PAD_NORMAL 0.0f   // every component of a padded vn / face_normals row

// number of live rows: the device count clamped into [0, capacity]; d_count == nullptr is the exact form (every row is live)
MVE_MCAP_FN int32_t mcap_live(int32_t capacity, const int32_t* d_count) {
    if (capacity < 0) capacity = 0;
    if (!d_count) return capacity;
    const int32_t c = *d_count;
    return c <= 0 ? 0 : (c < capacity ? c : capacity);
}

MVE_MCAP_FN int32_t mcap_overflow(int64_t n_verts, int64_t n_faces, int32_t v_cap, int32_t f_cap) {
    return (n_verts > (int64_t)v_cap || n_faces > (int64_t)f_cap) ? 1 : 0;
}

// what the extraction publishes: the true totals, the live counts (all or nothing) and the flag
MVE_MCAP_FN void mcap_resolve(int32_t n_verts, int32_t n_faces, int32_t v_cap, int32_t f_cap, int32_t* counts, int32_t* live, int32_t* overflow) {
    const int32_t ov = mcap_overflow(n_verts, n_faces, v_cap, f_cap);
    counts[0] = n_verts;
    counts[1] = n_faces;
    live[0] = ov ? 0 : mcap_live(v_cap, &n_verts);
    live[1] = ov ? 0 : mcap_live(f_cap, &n_faces);
    *overflow = ov;
}

// number of `block`-row blocks that hold at least one live row
MVE_MCAP_FN uint32_t mcap_blocks(int32_t live, int32_t block) { return live <= 0 ? 0u : ((uint32_t)live + (uint32_t)block - 1u) / (uint32_t)block; }

// does a run of `n` rows starting at `row` lie inside the live rows? (a tet's one or two faces)
MVE_MCAP_FN bool mcap_rows_fit(uint64_t row, uint32_t n, int32_t live) { return live > 0 && row + (uint64_t)n <= (uint64_t)(uint32_t)live; }
