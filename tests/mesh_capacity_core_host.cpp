// TEST INFRASTRUCTURE ONLY.  Stand-alone host walk of mvedit_amd/csrc/mesh_capacity_core.h -- the bounds arithmetic of the capacity form of
// the mesh optimisation iteration -- built by tests/test_mesh_capacity.py with -fsanitize=address,undefined and run as a program of its own.
// Every buffer is a heap block of exactly the size the contract promises (v_cap vertex rows, f_cap face rows), so a write the rules do
// not allow is an AddressSanitizer report, not a wrong number.  The walk does what mve_dmtet_extract_n does with one thread per row:
// resolve the counts, write the live rows under the kernels' guards, pad the rest.
//
// stdin : T, then per case:  n_verts n_faces v_cap f_cap garbage_v garbage_f
// stdout: per case one line: counts[0] counts[1] live[0] live[1] overflow written_v written_f padded_v padded_f stale blocks clamp_v clamp_f
//         then one line per probe of mcap_live (see main)
#include <cstdio>
#include <cstdlib>

#include "../mvedit_amd/csrc/mesh_capacity_core.h"

int main() {
    int T;
    if (scanf("%d", &T) != 1) return 2;
    const float STALE_F = 12345.0f;
    const int32_t STALE_I = 777777;
    for (int t = 0; t < T; ++t) {
        long long nv, nf, v_cap, f_cap, gv, gf;
        if (scanf("%lld %lld %lld %lld %lld %lld", &nv, &nf, &v_cap, &f_cap, &gv, &gf) != 6) return 2;
        float* verts = (float*)malloc(sizeof(float) * 3 * (size_t)v_cap);
        int32_t* edges = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)v_cap);
        int32_t* faces = (int32_t*)malloc(sizeof(int32_t) * 3 * (size_t)f_cap);
        for (long long i = 0; i < 3 * v_cap; ++i) verts[i] = STALE_F;
        for (long long i = 0; i < 2 * v_cap; ++i) edges[i] = STALE_I;
        for (long long i = 0; i < 3 * f_cap; ++i) faces[i] = STALE_I;
        int32_t counts[2], live[2], overflow;
        mcap_resolve((int32_t)nv, (int32_t)nf, (int32_t)v_cap, (int32_t)f_cap, counts, live, &overflow);
        // k_interp_verts: row k of the nv the extraction found is written when it is below the live count
        const int32_t lim_v = mcap_live((int32_t)v_cap, &live[0]);
        for (long long k = 0; k < nv; ++k) {
            if (k >= lim_v) break;
            for (int c = 0; c < 3; ++c) verts[3 * k + c] = 1.0f;
            edges[2 * k] = 1; edges[2 * k + 1] = 2;
        }
        // k_emit_faces: a tet owns a run of one or two rows and writes it when the whole run is live
        const int32_t lim_f = mcap_live((int32_t)f_cap, &live[1]);
        for (long long row = 0, run = 1; row < nf; row += run, run = 3 - run) {
            const long long n = row + run <= nf ? run : nf - row;
            if (!mcap_rows_fit((uint64_t)row, (uint32_t)n, lim_f)) continue;
            for (long long r = row; r < row + n; ++r)
                for (int c = 0; c < 3; ++c) faces[3 * r + c] = 1;
        }
        // k_dmtet_pad
        for (long long i = 0; i < v_cap; ++i)
            if (i >= mcap_live((int32_t)v_cap, &live[0])) {
                for (int c = 0; c < 3; ++c) verts[3 * i + c] = MVE_MCAP_PAD_VERT;
                edges[2 * i] = edges[2 * i + 1] = MVE_MCAP_PAD_INDEX;
            }
        for (long long i = 0; i < f_cap; ++i)
            if (i >= mcap_live((int32_t)f_cap, &live[1]))
                for (int c = 0; c < 3; ++c) faces[3 * i + c] = MVE_MCAP_PAD_INDEX;
        long long wv = 0, wf = 0, pv = 0, pf = 0, stale = 0;
        for (long long i = 0; i < v_cap; ++i) {
            const bool w = verts[3 * i] == 1.0f && verts[3 * i + 1] == 1.0f && verts[3 * i + 2] == 1.0f && edges[2 * i] == 1 && edges[2 * i + 1] == 2;
            const bool p = verts[3 * i] == 0.0f && verts[3 * i + 1] == 0.0f && verts[3 * i + 2] == 0.0f && edges[2 * i] == 0 && edges[2 * i + 1] == 0;
            wv += w; pv += p; stale += !(w || p);
        }
        for (long long i = 0; i < f_cap; ++i) {
            const bool w = faces[3 * i] == 1 && faces[3 * i + 1] == 1 && faces[3 * i + 2] == 1;
            const bool p = faces[3 * i] == 0 && faces[3 * i + 1] == 0 && faces[3 * i + 2] == 0;
            wf += w; pf += p; stale += !(w || p);
        }
        const int32_t g0 = (int32_t)gv, g1 = (int32_t)gf;
        printf("%d %d %d %d %d %lld %lld %lld %lld %lld %u %d %d\n", counts[0], counts[1], live[0], live[1], overflow, wv, wf, pv, pf, stale,
               mcap_blocks(live[0], 256), mcap_live((int32_t)v_cap, &g0), mcap_live((int32_t)f_cap, &g1));
        free(faces);
        free(edges);
        free(verts);
    }
    // mcap_live clamps any device count into [0, capacity]; no count = every row; a negative capacity is no rows
    const int32_t probes[] = {-2147483647 - 1, -5, 0, 1, 6, 7, 8, 2147483647};
    for (int32_t c : probes) printf("%d %d %d %d\n", mcap_live(7, &c), mcap_live(0, &c), mcap_live(1, &c), mcap_live(-3, &c));
    printf("%d %d %u %u %u %u\n", mcap_live(7, nullptr), mcap_live(-3, nullptr), mcap_blocks(0, 256), mcap_blocks(-4, 256), mcap_blocks(256, 256),
           mcap_blocks(257, 256));
    return 0;
}
