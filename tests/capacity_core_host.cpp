// TEST INFRASTRUCTURE ONLY.  Stand-alone host walk of mvedit_amd/csrc/capacity_core.h -- the bounds arithmetic of the capacity form of
// the NeRF training iteration -- built by tests/test_nerf_capacity.py with -fsanitize=address,undefined and run as a program of its own.
// Every buffer is a heap block of exactly the size the contract promises (the ray table 2 N ints, pref live + 1 ints), so a read the
// rules do not allow is an AddressSanitizer report, not a wrong number.
//
// stdin : T, then per case:  N capacity  cnt[0..N)  keep[0..capacity) (0 / 1)
// stdout: per case one line: total count deciders overflow live kept  o_off[0] o_cnt[0] ... o_off[N-1] o_cnt[N-1]
//         then one line per probe of cap_live (see main)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mvedit_amd/csrc/capacity_core.h"

int main() {
    int T;
    if (scanf("%d", &T) != 1) return 2;
    for (int t = 0; t < T; ++t) {
        long long N, capacity;
        if (scanf("%lld %lld", &N, &capacity) != 2) return 2;
        int32_t* rays = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)N);
        long long total = 0;
        for (long long n = 0; n < N; ++n) {
            int c;
            if (scanf("%d", &c) != 1) return 2;
            rays[2 * n] = (int32_t)total;
            rays[2 * n + 1] = c;
            total += c;
        }
        std::vector<int> keep((size_t)capacity);
        for (long long i = 0; i < capacity; ++i)
            if (scanf("%d", &keep[(size_t)i]) != 1) return 2;
        // clamp: what k_march_clamp does with one thread per ray
        int32_t count = 0;
        int deciders = 0;
        for (long long n = 0; n < N; ++n) {
            int32_t c;
            if (cap_clamp_decides(rays, (uint32_t)n, (uint32_t)N, (uint32_t)capacity, &c)) { count = c; ++deciders; }
        }
        const int overflow = total > capacity ? 1 : 0;
        const uint32_t live = cap_live((uint32_t)capacity, &count);
        // cull: pref over the live rows only, then k_cull_rays
        int32_t* pref = (int32_t*)malloc(sizeof(int32_t) * ((size_t)live + 1));
        int32_t kept = 0;
        for (uint32_t i = 0; i < live; ++i) { pref[i] = kept; kept += keep[i] ? 1 : 0; }
        pref[live] = kept;
        printf("%lld %d %d %d %u %d", total, count, deciders, overflow, live, kept);
        for (long long n = 0; n < N; ++n) {
            int32_t o, c;
            cap_cull_ray(rays[2 * n], rays[2 * n + 1], live, pref, &o, &c);
            printf(" %d %d", o, c);
        }
        printf("\n");
        free(pref);
        free(rays);
    }
    // cap_live clamps any device count into [0, capacity]; no count = every row
    const int32_t probes[] = {-2147483647 - 1, -5, 0, 1, 6, 7, 8, 2147483647};
    for (int32_t c : probes) printf("%u %u %u\n", cap_live(7u, &c), cap_live(0u, &c), cap_live(1u, &c));
    printf("%u\n", cap_live(7u, nullptr));
    return 0;
}
