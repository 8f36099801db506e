// Bounds arithmetic of the capacity (host-read-free) form of the NeRF training iteration: which samples and which rays exist when the
// sample tensors are sized by a caller-chosen CAPACITY and the number of live samples is a count in device memory.  Used by
// raymarching.hip, nerf.hip and recon_loss.hip; the same source compiles for the host, where tests/test_nerf_capacity.py walks it
// under the address and undefined-behaviour sanitizers against a Python restatement of the rules below.
//
// Rules.  The ray table rays[n] = (offset, count) is an exclusive prefix sum in ray order (mve_march_rays_train_count), so ray ends
// offset + count never decrease with n.
//   * a ray FITS a capacity when offset + count <= capacity (the test k_march_write and the composite kernels already apply);
//   * the live count after the march is the largest end of a fitting ray: the samples of the longest prefix of whole rays that fit
//     (= the marched total when nothing overflows, 0 when not even ray 0 fits);
//   * a sample index exists when it is below min(max(count, 0), capacity);
//   * weight culling re-indexes a ray through the prefix counts pref[0 .. count] only when offset + count <= live count; any other ray
//     becomes (pref[live count], 0): it did not fit, it keeps no samples, and pref is never read past the live count.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MVE_CAP_FN __host__ __device__ __forceinline__
#else
#define MVE_CAP_FN static inline
#endif

// number of live samples: the device count clamped into [0, capacity]; d_count == nullptr is the exact form (every row is live)
MVE_CAP_FN uint32_t cap_live(uint32_t capacity, const int32_t* d_count) {
    if (!d_count) return capacity;
    const int32_t c = *d_count;
    return c <= 0 ? 0u : ((uint32_t)c < capacity ? (uint32_t)c : capacity);
}

MVE_CAP_FN bool cap_ray_fits(int32_t off, int32_t cnt, uint32_t limit) {
    return off >= 0 && cnt >= 0 && (uint64_t)(uint32_t)off + (uint64_t)(uint32_t)cnt <= (uint64_t)limit;
}

// Clamp step, one call per ray n of N: returns true when ray n is the one that decides the live count, which is then *count.
// Ends never decrease, so exactly one ray decides: the last fitting ray (its successor does not fit, or there is none), or ray 0 when
// it does not fit itself (count 0).
MVE_CAP_FN bool cap_clamp_decides(const int32_t* rays, uint32_t n, uint32_t N, uint32_t capacity, int32_t* count) {
    const bool fits = cap_ray_fits(rays[2ull * n], rays[2ull * n + 1], capacity);
    if (!fits) {
        if (n != 0) return false;
        *count = 0;
        return true;
    }
    if (n + 1 < N && cap_ray_fits(rays[2ull * (n + 1)], rays[2ull * (n + 1) + 1], capacity)) return false;
    *count = rays[2ull * n] + rays[2ull * n + 1];
    return true;
}

// Cull re-index of one ray: pref [live + 1 entries read at most] = exclusive prefix count of kept samples, pref[live] = kept total.
MVE_CAP_FN void cap_cull_ray(int32_t off, int32_t cnt, uint32_t live, const int32_t* pref, int32_t* o_off, int32_t* o_cnt) {
    if (cap_ray_fits(off, cnt, live)) {
        const int32_t a = pref[off], b = pref[off + cnt];
        *o_off = a;
        *o_cnt = b - a;
    } else {
        *o_off = pref[live];
        *o_cnt = 0;
    }
}
