// Host-side dispatch of the GEMM / implicit-GEMM conv kernels: the switches, the eligibility predicates and the ONE function that decides which
// kernel a launch gets (gemm_plan).  Plain C++: no HIP runtime call, no device code -- it compiles with any host compiler against gemm_shared.h's parameter structs,
// so the decision can be swept and sanitized without a GPU.  gemm.hip computes the plan and launches from it; the launchers of the three kernel
// files (gemm.hip: 128-row kernel; gemm_big.hip: 256-row two-stage loop; gemm_pp.hip: 256-row ping-pong loop) launch exactly what the plan names.
// Every kernel produces bit-identical results (same K order, same epilogue arithmetic), so the plan is free to choose by problem size.
#pragma once
#include <stdlib.h>

#include "gemm_shared.h"

namespace {

// The switches.  One process-wide instance (gemm.hip: gemm_switches()), read from the environment on first use of any GEMM entry point or tune
// call -- not at library load: tools set the environment after import.  The mve_gemm_*_tune entry points pack / unpack it.
struct GemmSwitches {
    // minimum number of 256 x 320 blocks for which the big-tile kernel is used (0 disables it); MVE_GEMM_BIG overrides
    int big_min_blocks = 256;     // one block per CU: measured break-even on MI355X (profiles/r01_ab_gemm_big*.log)
    int seq_splitk = 1;           // mve_gemm_tune bit 29 clears it (A/B: real split-K + reducer)
    // What a launch does when the slice rule (choose_splitk) asks for S > 1 slices but the un-split launch already fills the chip (>= one 256 x 320
    // tile per CU: 64 images on one GPU at the 32 x 32 and 16 x 16 levels).
    //   0 (default, round 4): one block per tile walks all of K in ONE accumulation chain.  The result differs from the sliced sum (what the same
    //     image gets in a small batch, where the slices run as separate blocks + reducer) by fp32 summation order only -- well inside the 16-bit output
    //     rounding, see tests/test_unet_ops.py::test_unsplit_chain_vs_sliced_sum -- so bitwise batch invariance holds among launches that take the
    //     same decision (all small batches; all chip-filling batches), not across the two.
    //   1 (MVE_GEMM_STRICT_SPLITK=1 / mve_gemm_tune bit 30): the block emulates the slices (GemmParams::splitk_seq: accumulators folded into an fp32
    //     running total at every slice boundary), bitwise equal to split-K + reducer at any batch.  Measured cost at 64 images: the fold drains
    //     the DMA ring and moves 160 fp32 registers per lane through HBM per slice: level-1 / level-2 convs 1 080 -> 1 310-1 400 TFLOP/s without it,
    //     the N = K GEMMs of level 2 550 -> 900, ff.out 750 -> 1 240; 3.8 ms of a 68 ms step (profiles/r04_oplist_*.log).
    int strict_splitk = 0;
    // The 256-row tile has two main loops with bit-identical results: the ping-pong schedule (gemm_pp.hip) wherever it is eligible,
    // else the two-stage loop (gemm_big.hip).  mve_gemm_tune bit 27 / MVE_GEMM_PP=0 turn the former off (A/B).
    int pp = 1;
    // The two-blocks-per-CU 256 x 160 tile (gemm_pp.hip, NSL = 3) for dense GEMMs, bit-identical results.  2 (default): taken where the dispatcher
    // asks for the narrow tile because 320-wide tiles would leave CUs idle (small batches: the per-wave epilogue and the second resident block are
    // what those short launches lack); 1: wherever it is eligible (A/B: slower at 64 images); 0: never.  MVE_GEMM_PP2 / mve_gemm_tune.
    int pp2 = 2;
    // A/B aid (mve_gemm_tune bit 25, no environment variable): 1 = the ring swizzle of round 2 ((row >> 2) & 3: every fragment read 2-way bank
    // conflicted); results are identical either way
    int old_swizzle = 0;
    // The four-stage ring of the 128-row kernel (k_gemm_deep) for launches of at most this many blocks; 0 turns it off.  MVE_GEMM_DEEP / mve_gemm_deep_tune.
    int deep_max_blocks = 0;
    // Weight-strip-major block order for launches whose activations are the smaller operand (GemmParams::w_major).  MVE_GEMM_WMAJOR=0 / mve_gemm_deep_tune bit 30 off.
    int w_major = 1;
    // In-kernel slice reduction (round 6; gemm_pp.hip: pp_reduce_slices).  A K-sliced launch that the ping-pong tile can take (320-wide where that fills
    // the chip, 160-wide otherwise) folds its slices inside the launch: no k_splitk_reduce launch behind it, and -- for the small launches of a rank
    // that holds few images, which used to run on the 128-row two-stage kernel -- the deep LDS-DMA ring of the ping-pong loop.  Bit-identical to
    // partials + reducer (same slices, same fold order, same epilogue function).  MVE_GEMM_RED=0 / mve_gemm_red_tune(0) restore the reducer launches.
    // bit 0: the 128-row kernel folds its slices (rule V1 of gemm_plan);  bit 1: small K-sliced launches go to the ping-pong tile and fold there (rule 3)
    int red = 0;      // off: measured slower than partials + reducer on every K-sliced launch of an 8-image forward but the longest (profiles/r06_fold_modes_8images.log)
    // Narrower tile for launches of at most small_bn_max 128 x 160 blocks (see v128_bn).  MVE_GEMM_SMALL_BN = 0 | 64 | 128, MVE_GEMM_SMALL_BN_MAX.
    int small_bn = 64;      // same-box sweep, profiles/r06_ab_small_bn.log: Zero123++ 21.55 -> 20.4 ms, 8-image forward -1 %; 128 is neutral
    int small_bn_max = 384;
    // 64 x 64 tiles where even the 128 x 64 tiling is at most small_bm_max blocks.  MVE_GEMM_SMALL_BM = 64 | 0, MVE_GEMM_SMALL_BM_MAX.
    int small_bm = 0;
    int small_bm_max = 512;
    // K columns per block from which a launch that fills neither 256-row rule takes the ping-pong 256 x 160 tile anyway; 0 = never.  MVE_GEMM_PP160_MINK.
    int pp160_min_k = 1440;      // same-box sweep, profiles/r06_ab_pp160_min_k.log: Zero123++ 22.9 -> 21.4 ms, 8-image forward 12.44 -> 12.18 ms; 640 and below lose again
    int splitk_policy = 1;       // MVE_GEMM_SPLITK: 1 (default) = the rule of choose_splitk; 0 = never split (A/B: what the slices cost at a given batch)
    int ln_fuse = 1;             // MVE_GEMM_LN_FUSE (default 1); 0: never (A/B, tests)
    // 1 (default; MVE_PHASES_ONE_LAUNCH): the four phases of mve_upsample_conv_phases run as one launch where a phase fills whole tiles; 0: always four launches
    int phases_one_launch = 1;
    // development switch MVE_PP_DBG (0 in every shipped path; GemmParams::dbg of the ping-pong launches).  Here because bit 1 -- pair launches of the
    // 256-row tile take the generic epilogue path -- vetoes the fused LayerNorm (pp_ln_fusable)
    int pp_dbg = 0;

    static GemmSwitches from_env() {
        GemmSwitches sw;
        auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        sw.big_min_blocks = env("MVE_GEMM_BIG", sw.big_min_blocks);
        sw.strict_splitk = env("MVE_GEMM_STRICT_SPLITK", 0) != 0;
        sw.pp = env("MVE_GEMM_PP", sw.pp);
        sw.pp2 = env("MVE_GEMM_PP2", sw.pp2);
        if (sw.pp2 < 0 || sw.pp2 > 2) sw.pp2 = 2;
        sw.deep_max_blocks = env("MVE_GEMM_DEEP", sw.deep_max_blocks);
        sw.w_major = env("MVE_GEMM_WMAJOR", sw.w_major);
        sw.red = env("MVE_GEMM_RED", sw.red);
        sw.small_bn = env("MVE_GEMM_SMALL_BN", sw.small_bn);
        if (sw.small_bn != 64 && sw.small_bn != 128) sw.small_bn = 0;
        sw.small_bn_max = env("MVE_GEMM_SMALL_BN_MAX", sw.small_bn_max);
        sw.small_bm = env("MVE_GEMM_SMALL_BM", sw.small_bm);
        if (sw.small_bm != 64) sw.small_bm = 0;
        sw.small_bm_max = env("MVE_GEMM_SMALL_BM_MAX", sw.small_bm_max);
        sw.pp160_min_k = env("MVE_GEMM_PP160_MINK", sw.pp160_min_k);
        sw.splitk_policy = env("MVE_GEMM_SPLITK", sw.splitk_policy);
        sw.ln_fuse = env("MVE_GEMM_LN_FUSE", sw.ln_fuse);
        sw.phases_one_launch = env("MVE_PHASES_ONE_LAUNCH", 1) != 0;
        sw.pp_dbg = env("MVE_PP_DBG", 0);
        return sw;
    }

    // ---- the tune words: bit positions named once; every setter returns the whole previous word, so that old = tune(x); ...; tune(old)
    // restores every switch of the word.  A negative argument only queries.
    enum : int {
        TUNE_OLD_SWIZZLE = 1 << 25,      // mve_gemm_tune
        TUNE_PP2_ALL = 1 << 26,          //   pp2 = 1
        TUNE_PP_OFF = 1 << 27,
        TUNE_PP2_OFF = 1 << 28,          //   pp2 = 0 (bit 26 wins when both are set)
        TUNE_REAL_SPLITK = 1 << 29,      //   seq_splitk = 0
        TUNE_STRICT_SPLITK = 1 << 30,
        TUNE_OPTION_BITS = TUNE_OLD_SWIZZLE | TUNE_PP2_ALL | TUNE_PP_OFF | TUNE_PP2_OFF | TUNE_REAL_SPLITK | TUNE_STRICT_SPLITK,
        DEEP_TUNE_W_MAJOR_OFF = 1 << 30, // mve_gemm_deep_tune
        RED_TUNE_MASK = 3,               // mve_gemm_red_tune
    };
    int tune_word() const {
        return big_min_blocks | (seq_splitk ? 0 : TUNE_REAL_SPLITK) | (pp ? 0 : TUNE_PP_OFF) | (pp2 == 1 ? TUNE_PP2_ALL : 0) | (pp2 == 0 ? TUNE_PP2_OFF : 0) |
               (old_swizzle ? TUNE_OLD_SWIZZLE : 0) | (strict_splitk ? TUNE_STRICT_SPLITK : 0);
    }
    void set_tune_word(int w) {
        strict_splitk = (w & TUNE_STRICT_SPLITK) ? 1 : 0;
        seq_splitk = (w & TUNE_REAL_SPLITK) ? 0 : 1;
        pp = (w & TUNE_PP_OFF) ? 0 : 1;
        pp2 = (w & TUNE_PP2_ALL) ? 1 : ((w & TUNE_PP2_OFF) ? 0 : 2);
        old_swizzle = (w & TUNE_OLD_SWIZZLE) ? 1 : 0;
        big_min_blocks = w & ~TUNE_OPTION_BITS;
    }
    int deep_tune_word() const { return deep_max_blocks | (w_major ? 0 : DEEP_TUNE_W_MAJOR_OFF); }
    void set_deep_tune_word(int w) { deep_max_blocks = w & ~DEEP_TUNE_W_MAJOR_OFF; w_major = (w & DEEP_TUNE_W_MAJOR_OFF) ? 0 : 1; }
};

// Eligibility predicates: pure functions of (mode, GemmParams, GemmSwitches).  mode 0: dense A, 1: conv gather.
constexpr int SK_SYNC_TILES = 8192;             // counters of the in-kernel slice fold (GemmParams::sk_sync): one per output tile
constexpr unsigned PP_NUMREC = 0xFFFFFF00u;     // buffer resource size of the ping-pong kernel: every valid offset is below it, the all-ones halo offset above

inline unsigned gemm_cdiv(unsigned long long a, unsigned long long b) { return (unsigned)((a + b - 1) / b); }
inline int gemm_slices(const GemmParams& p) { return p.splitk > 1 ? p.splitk : 1; }

// Split K at the deep UNet levels, where one image contributes only a few output tiles (8x8 / 16x16 latents) but K is
// 9*1280..9*2560.  The RULE below is a function of (rows per image, N, K) only -- never of the batch.  What a launch actually runs with is the
// rule's count only while the launch is small: gemm_plan (below) runs ONE accumulation chain where the un-split launch fills the chip and
// `ceil(256 / tiles)` slices where the rule would over-fill it, so the effective count falls with the rows of the launch
// (mve_gemm_effective_splitk; 16 x 16 level: 4 slices up to 16 images, 2 at 32, 1 from 64; 8 x 8 level: 8 / 4 / 2 / 1 slices at <= 32 / 64 / 128 /
// 256 images).  A view therefore gets bit-identical results alone, in a chunk or on another rank AS LONG AS those launches take the same decision
// (all small batches do); MVE_GEMM_STRICT_SPLITK=1 / mve_gemm_tune bit 30 / mvedit_amd.parallel.set_partition_invariant() make every launch
// round as the rule's slices, at any batch (tests/test_abi.py::test_effective_splitk_by_batch).
inline int choose_splitk(int rows_per_image, int N, int K, const GemmSwitches& sw) {
    if (rows_per_image <= 0 || sw.splitk_policy == 0) return 1;
    const int bn = (N % 160 == 0) ? 160 : (N % 128 == 0 ? 128 : (N <= 64 ? 64 : 128));
    const long long t1 = (long long)gemm_cdiv(rows_per_image, 128) * gemm_cdiv(N, bn);      // tiles of ONE image
    const int nk = (K + BK - 1) / BK;
    // ceil (round 6): an image of 40 tiles (the 30 x 20 level of Zero123++'s 120 x 80 latent: 80 blocks for a CFG pair, each walking K = 11 520 alone --
    // 271 us per conv, profiles/r06_trace_zero123pp.txt) gets 2 slices instead of 1.  Power-of-two tile counts (every level of a 64 x 64 latent: 64 / 32 /
    // 16 / 8 tiles) divide 64: their slice counts, and with them every bit of those results, are unchanged.
    long long s = (64 + t1 - 1) / t1;
    if (s > nk / 8) s = nk / 8;        // at least 8 K tiles (512 k) per slice
    if (s > 16) s = 16;
    return s < 2 ? 1 : (int)s;
}

// Width of the 256-row tile for N columns (0: none fits): 320 (every UNet width), 256 (the VAE's 256 / 512-channel convs; no
// split-K variants), 128 (the VAE's 128-channel convs at image resolution; ping-pong loop only, no split-K).  Any other N -- 8 for
// conv_out -- would leave most of a tile dead and takes the 128 x {64,128,160} kernel, whose results are bit-identical.
inline int tile256_bn(int N, int splitk, const GemmSwitches& sw) {
    if (N % 320 == 0) return 320;
    if (splitk > 1) return 0;
    if (N % 256 == 0) return 256;
    if (N % 128 == 0 && sw.pp) return 128;
    return 0;
}
inline long long blocks256(int bn, int M, int N, int splitk) { return (bn == 0 || M < 64) ? 0 : (long long)gemm_cdiv(M, 256) * (N / bn) * (splitk > 1 ? splitk : 1); }
inline long long tile256_blocks(int M, int N, int splitk, const GemmSwitches& sw) { return blocks256(tile256_bn(N, splitk, sw), M, N, splitk); }

// The two-stage 256-row loop (gemm_big.hip): tile width 320 (wave tile 128 x 80, every UNet width is a multiple of 320) or 256 (the VAE's
// 256 / 512-channel convolutions; no split-K variants), and the number of blocks it would launch (0: shape not eligible)
inline int big_bn(int N) { return N % 320 == 0 ? 320 : (N % 256 == 0 ? 256 : 0); }
inline long long big_blocks(int M, int N, int splitk) { return blocks256(big_bn(N) == 256 && splitk > 1 ? 0 : big_bn(N), M, N, splitk); }

// The ping-pong 256-row loop (gemm_pp.hip).  Every per-lane byte offset must stay below the resource size (and the out-of-range marker above it)
inline bool pp_fits(unsigned long long bytes) { return bytes + 65536ull < (unsigned long long)PP_NUMREC; }
inline int pp_bn(int N) { return N % 320 == 0 ? 320 : (N % 256 == 0 ? 256 : (N % 128 == 0 ? 128 : 0)); }
inline int pp_bn(const GemmParams& p) { return (p.tile_n == 160 && p.N % 160 == 0) ? 160 : pp_bn(p.N); }

inline bool pp_eligible(int mode, const GemmParams& p) {
    const int bn = pp_bn(p);
    if (bn == 0 || p.M < 64 || p.K % BK != 0) return false;
    if (bn != 320 && bn != 160 && p.splitk > 1) return false;
    if (bn != 320 && p.splitk_seq > 1) return false;
    if (!pp_fits((unsigned long long)p.N * p.ldw * 2)) return false;
    if (mode == 0) return pp_fits((unsigned long long)p.M * p.lda * 2);
    if (!p.g.chunk64) return false;
    const int hw = p.g.Ho * p.g.Wo;
    if (p.g.phase_rows > 0 && (p.g.kw != 2 || p.g.phase_rows % 256 != 0 || p.M != 4 * p.g.phase_rows)) return false;
    const int m_img = p.g.phase_rows > 0 ? p.g.phase_rows : p.M;      // rows that address distinct source pixels
    const unsigned long long px = (unsigned long long)(((long long)m_img + hw - 1) / hw) * p.g.Hs * p.g.Ws + 2ull * p.g.Ws + 4;
    int cmax = p.g.C1 > p.g.C2 ? p.g.C1 : p.g.C2;
    cmax = cmax > p.g.C3 ? cmax : p.g.C3;
    cmax = cmax > p.g.C4 ? cmax : p.g.C4;
    return pp_fits(px * cmax * 2);
}

// The two-blocks-per-CU tile: dense GEMM, whole 256 x 160 tiles, the epilogue configuration pp2_epilogue implements
inline bool pp2_eligible(int mode, const GemmParams& p) {
    if (mode != 0 || p.N % 160 != 0 || p.M % 256 != 0 || p.K % BK != 0) return false;
    if (p.splitk > 1 || p.splitk_seq > 1 || p.rowvec || p.out_f32 || p.out_scale != 1.0f || (p.residual && p.res_after_scale)) return false;
    if (p.residual_lo || p.out_lo) return false;          // the pair epilogue lives in big_tile_epilogue / gemm_epilogue_tail only
    if (p.ldc % 8 != 0) return false;
    return pp_fits((unsigned long long)p.N * p.ldw * 2) && pp_fits((unsigned long long)p.M * p.lda * 2);
}

// LayerNorm of the output rows inside the launch (GemmParams::ln_out): exactly the configuration big_tile_epilogue's pair fast path takes on EVERY
// tile of the launch
inline bool pp_ln_fusable(const GemmParams& p, const GemmSwitches& sw) {
    return sw.ln_fuse != 0 && p.N == 320 && p.M % 256 == 0 && p.out_lo && p.bias && p.out_scale == 1.0f && !p.res_after_scale && !p.out_f32 && !p.geglu &&
           !p.rowvec && p.splitk <= 1 && p.splitk_seq <= 1 && p.orow_extra == 0 && p.tile_n == 0 && !(sw.pp_dbg & 2) && p.ln_gamma && p.ln_beta && p.ld_ln % 8 == 0;
}

// Tile width of the 128-row kernel: prefer the widest tile that divides N (no dead columns), else 128
inline int v128_bn(const GemmParams& p, const GemmSwitches& sw) {
    int bn = 128;
    if (p.N % 160 == 0) bn = 160;
    else if (p.N % 128 == 0) bn = 128;
    else if (p.N <= 64) bn = 64;
    // (round 6) a launch of at most one 128 x 160 block per CU runs its phases back to back (one wave per SIMD: LDS-DMA, fragment reads + MFMAs and
    // the epilogue add up, profiles/r06_gemm_lab_ablation.txt); narrower tiles put two or more blocks on a CU, whose phases overlap.  sw.small_bn:
    // the tile width such launches take when it divides N (0 = keep 160).  Bit-identical like every tile choice.
    if (bn == 160 && sw.small_bn > 0 && p.N % sw.small_bn == 0 &&
        gemm_cdiv(p.M, 128) * gemm_cdiv(p.N, 160) * gemm_slices(p) <= (unsigned)sw.small_bn_max)
        bn = sw.small_bn;
    return bn;
}

// The plan: what ONE launch of the dispatcher runs.
enum GemmFamily { GEMM_V128 = 0, GEMM_BIG = 1, GEMM_PP = 2, GEMM_PP2 = 3 };      // gemm.hip | gemm_big.hip | gemm_pp.hip four slots | gemm_pp.hip three slots, two blocks per CU
enum GemmRing { GEMM_RING_TWO_STAGE = 0, GEMM_RING_DEEP = 1, GEMM_RING_PINGPONG = 2 };      // k_gemm / k_gemm64 / k_gemm_big | k_gemm_deep | k_gemm_pp
enum GemmEpilogue {
    GEMM_EPI_PLAIN = 0,      // fused epilogue, or raw fp32 partials when K is sliced (the 128-row kernel carries a residual pair here too)
    GEMM_EPI_PAIR = 1,       // ping-pong tile, residual_pair instantiation
    GEMM_EPI_RED = 2,        // K slices folded inside the launch (GemmParams::sk_sync): no reducer launch
    GEMM_EPI_LNF = 3,        // ping-pong 320-wide pair tile that also normalises its rows (GemmParams::ln_out)
    GEMM_EPI_SEQ = 4,        // one block emulates splitk_seq slices (GemmParams::splitk_seq)
};
enum GemmPlanError {
    GEMM_PLAN_OK = 0,
    GEMM_PLAN_ERR_WINDOW = 1,      // a 2 x 2 conv window reached the 128-row kernel
    GEMM_PLAN_ERR_PP_ONLY = 2,     // pp_only and the ping-pong kernel does not take the problem
};

struct GemmPlan {
    int error;               // GemmPlanError; everything below is meaningless unless GEMM_PLAN_OK
    int family;              // GemmFamily
    int tile_n, tile_m;      // tile width 320 / 256 / 160 / 128 / 64 and rows 256 / 128 / 64
    int ring;                // GemmRing
    int epilogue;            // GemmEpilogue
    int splitk, splitk_seq;  // what GemmParams::splitk / splitk_seq of the launch are
    int reducer;             // 1: a k_splitk_reduce launch follows
    int w_major;             // block order (GemmParams::w_major, decided where the parameters are filled)
    unsigned grid;           // blocks of the GEMM launch
};

inline GemmPlan plan_error(int e) { GemmPlan pl = {}; pl.error = e; return pl; }
inline GemmPlan plan_of(int family, int bn, int bm, int ring, int epilogue, const GemmParams& q) {
    GemmPlan pl = {};
    pl.family = family; pl.tile_n = bn; pl.tile_m = bm; pl.ring = ring; pl.epilogue = epilogue;
    pl.splitk = q.splitk; pl.splitk_seq = q.splitk_seq;
    pl.reducer = q.splitk > 1 && epilogue != GEMM_EPI_RED;
    pl.w_major = q.w_major;
    pl.grid = gemm_cdiv(q.M, bm) * gemm_cdiv(q.N, bn) * (unsigned)gemm_slices(q);
    return pl;
}

// the partial tiles of a fold are addressed through 32-bit buffer offsets
inline bool fold_offsets_fit(const GemmParams& q) { return (unsigned long long)q.splitk * q.M * q.N * 4ull < 0xF0000000ull; }

// Does the ping-pong four-slot loop take q as it stands (tile width pp_bn(q)), and with which epilogue instantiation?  `fold`: the launch folds its
// K slices (the caller holds the counters).  The slice fold and the residual pair exist for the 320- and 160-wide tiles without slice emulation only.
inline bool pp_takes(int mode, const GemmParams& q, const GemmSwitches& sw, bool fold, int* epilogue) {
    if (!pp_eligible(mode, q)) return false;
    const int bn = pp_bn(q);
    const bool seq = q.splitk_seq > 1, wide = bn == 320 || bn == 160;
    if (fold && q.splitk > 1) { *epilogue = GEMM_EPI_RED; return !seq && wide; }      // (the partial tiles leave raw: the plain instantiation's generic epilogue path)
    if (!seq && bn == 320 && mode == 0 && q.ln_out && pp_ln_fusable(q, sw)) { *epilogue = GEMM_EPI_LNF; return true; }
    if (q.residual_lo || q.out_lo) { *epilogue = GEMM_EPI_PAIR; return !seq && wide; }      // residual_pair mode: the 320-wide and (round 5: small batches) 160-wide tiles; else the 128-row kernel, whose gemm_epilogue_tail carries the pair
    *epilogue = seq ? GEMM_EPI_SEQ : GEMM_EPI_PLAIN;
    return true;
}

// A K-sliced launch on the ping-pong tile with the slices folded inside the launch (sw.red bit 1).  q.tile_n is set for the tile taken.
inline bool plan_pp_fold(int mode, GemmParams q, const GemmSwitches& sw, bool fold_buffer_available, GemmPlan* pl) {
    if (!(sw.red & 2) || !sw.pp || q.splitk <= 1 || q.splitk > 64 || q.M < 64) return false;
    const long long tm = gemm_cdiv(q.M, 256);
    if (q.N % 320 == 0 && tm * (q.N / 320) * q.splitk >= 256) q.tile_n = 0;
    else if (q.N % 160 == 0) q.tile_n = 160;
    else return false;
    const long long tiles = tm * (q.N / (q.tile_n == 160 ? 160 : 320));
    if (tiles > SK_SYNC_TILES || tiles * q.splitk > 256) return false;      // every block of the grid resident at once (one 104-144 KiB block per CU): a block waiting for its siblings never holds the slot one of them needs
    if (!fold_offsets_fit(q) || !fold_buffer_available) return false;
    int epi;
    if (!pp_takes(mode, q, sw, true, &epi)) return false;
    *pl = plan_of(GEMM_PP, pp_bn(q), 256, GEMM_RING_PINGPONG, epi, q);
    return true;
}

// The 256-row tile for q as it stands (q.tile_n = 160: the narrow tile is asked for): the three-slot tile, the four-slot ping-pong loop, the
// two-stage loop, in this order.  false: none takes it.
inline bool plan_tile256(int mode, const GemmParams& q, const GemmSwitches& sw, GemmPlan* pl) {
    // (round 6) in the default mode also the chip-filling launches WITHOUT a GEGLU epilogue: attn1.qkv / attn2.to_q at every level run 8-16 % faster on
    // two 256 x 160 blocks per CU than on one 256 x 320 block (the epilogue of one block under the K loop of the other; K = C is 10-40 steps), the
    // GEGLU launches 6-7 % slower at the 32 x 32 level (profiles/r06_oplist64_pp2_ab.txt) -- residual / pair launches are not eligible for this tile
    if (sw.pp && mode == 0 && q.splitk <= 1 && q.splitk_seq <= 1 &&
        ((sw.pp2 == 1 && q.tile_n == 0) || (sw.pp2 == 2 && (q.tile_n == 160 || (q.tile_n == 0 && !q.geglu)))) && pp2_eligible(mode, q)) {
        *pl = plan_of(GEMM_PP2, 160, 256, GEMM_RING_PINGPONG, GEMM_EPI_PLAIN, q);
        return true;
    }
    int epi;
    if (sw.pp && pp_takes(mode, q, sw, false, &epi)) {
        *pl = plan_of(GEMM_PP, pp_bn(q), 256, GEMM_RING_PINGPONG, epi, q);
        return true;
    }
    if (q.tile_n == 160 || big_blocks(q.M, q.N, q.splitk) <= 0) return false;
    if (q.residual_lo || q.out_lo) return false;        // residual_pair mode: only the ping-pong 320-wide tile and the 128-row kernel carry the pair
    *pl = plan_of(GEMM_BIG, big_bn(q.N), 256, GEMM_RING_TWO_STAGE, q.splitk_seq > 1 ? GEMM_EPI_SEQ : GEMM_EPI_PLAIN, q);
    return true;
}

// The 128-row kernel (gemm.hip): it takes everything but 2 x 2 conv windows.
inline GemmPlan plan_v128(const GemmParams& q, const GemmSwitches& sw, bool fold_buffer_available) {
    if (q.g.kw == 2) return plan_error(GEMM_PLAN_ERR_WINDOW);      // 2 x 2 conv windows run on the ping-pong kernel only
    const int bn = v128_bn(q, sw);
    const unsigned tiles_m = gemm_cdiv(q.M, 128), tiles_n = gemm_cdiv(q.N, bn);
    const unsigned grid = tiles_m * tiles_n * gemm_slices(q);
    // V1. K slices folded inside the launch (gemm_reduce_slices; sw.red bit 0) where every block of the grid is resident at once -- two 72 KiB blocks
    // per CU -- so that a block waiting for its siblings never holds the slot one of them needs: no k_splitk_reduce launch behind such a launch
    const int epi = (q.splitk > 1 && (sw.red & 1) && grid <= 512 && tiles_m * tiles_n <= (unsigned)SK_SYNC_TILES && fold_offsets_fit(q) && fold_buffer_available)
                        ? GEMM_EPI_RED : GEMM_EPI_PLAIN;
    // V2. launches of at most sw.deep_max_blocks blocks (a block or two per CU) and more than two K tiles per block: the four-stage ring (k_gemm_deep)
    const int nk_slice = ((q.K + BK - 1) / BK) / gemm_slices(q);
    if ((int)grid <= sw.deep_max_blocks && nk_slice > 2 && bn >= 128) return plan_of(GEMM_V128, bn, 128, GEMM_RING_DEEP, epi, q);
    // V3. ... and 64 x 64 tiles where even the 128 x 64 tiling is at most sw.small_bm_max blocks (MVE_GEMM_SMALL_BM = 64 | 0)
    if (bn == 64 && sw.small_bm == 64 && q.N % 64 == 0 && q.M > 64 && (int)grid <= sw.small_bm_max) return plan_of(GEMM_V128, 64, 64, GEMM_RING_TWO_STAGE, epi, q);
    // V4. the two-stage 128 x bn kernel
    return plan_of(GEMM_V128, bn, 128, GEMM_RING_TWO_STAGE, epi, q);
}

// Rule 2 of gemm_plan: just enough K slices for one block per CU where the slice rule's S would over-fill the chip (t1: 256 x 320 tiles un-split)
inline int few_slices(long long t1, int S, int minb) {
    if (S <= 2 || t1 <= 0 || t1 * S < 2 * minb) return S;
    const int few = (int)((minb + t1 - 1) / t1);
    return few < 2 ? 2 : (few < S ? few : S);
}

// The ONE place that decides.  The rules are tried in order; the first that takes the launch wins.
//   fold_buffer_available: the caller holds the slice-fold counters (gemm.hip: gemm_sk_sync -- its allocation can fail under stream capture, which is
//     the one impure step of the decision; the caller tries only when sw.red asks for a fold)
//   pp_only: the launch exists on the ping-pong loop alone (the 2 x 2 phase convs of mve_upsample_conv_phases): an error instead of the other loops
inline GemmPlan gemm_plan(int mode, const GemmParams& p, const GemmSwitches& sw, bool fold_buffer_available, bool pp_only) {
    GemmParams q = p;
    GemmPlan pl;
    int epi;
    if (pp_only) {
        // One K-sliced launch of a phase of mve_upsample_conv_phases: the slice policy of rules 1-3 on the ping-pong kernel alone.
        const int minb = sw.big_min_blocks > 0 ? sw.big_min_blocks : 256;
        if (q.splitk > 1 && q.N % 320 != 0) q.splitk = 1;         // (only the 320-wide tile cuts K)
        // (strict mode, MVE_GEMM_STRICT_SPLITK: the rule's slices run as real slices + reducer at any batch -- the path small batches take anyway; the
        // in-block slice emulation of the 3 x 3 convs is not instantiated for this form)
        if (q.splitk > 1 && !sw.strict_splitk) {
            const long long t1 = tile256_blocks(q.M, q.N, 1, sw);
            q.splitk = t1 >= minb ? 1 : few_slices(t1, q.splitk, minb);      // the un-split launch fills the chip: one accumulation chain; else rule 2
        }
        if (plan_pp_fold(mode, q, sw, fold_buffer_available, &pl)) return pl;
        if (!pp_takes(mode, q, sw, false, &epi)) return plan_error(GEMM_PLAN_ERR_PP_ONLY);
        return plan_of(GEMM_PP, pp_bn(q), 256, GEMM_RING_PINGPONG, epi, q);
    }
    const int minb = sw.big_min_blocks;
    // 0. No 256-row tile width divides N: the 128-row kernel.
    if (tile256_bn(q.N, q.splitk, sw) == 0) return plan_v128(q, sw, fold_buffer_available);
    // 1. Enough 256 x 320 tiles to fill the chip WITHOUT cutting K: one block per tile walks all of K -- in ONE accumulation chain by default, slice
    // by slice in the strict mode, which reproduces the split-K rounding exactly (GemmParams::splitk_seq) -- no partial tiles, no reducer launch
    // (see GemmSwitches::strict_splitk).
    if (minb > 0 && q.splitk > 1 && q.N % 320 == 0 && sw.seq_splitk && tile256_blocks(q.M, q.N, 1, sw) >= minb &&
        (size_t)tile256_blocks(q.M, q.N, 1, sw) * 256 * 320 <= (size_t)q.splitk * q.M * q.N) {
        GemmParams c = q;
        c.splitk_seq = sw.strict_splitk ? q.splitk : 0;
        c.splitk = 1;
        if (plan_tile256(mode, c, sw, &pl)) return pl;      // else no 256-row loop takes it in this form (e.g. strict slices + residual pair): split K for real below
    }
    // 2. The slice rule asks for more slices than this launch needs to fill the chip (64 images at the 8 x 8 level: 64 tiles x 8 slices): cut K into
    // just enough slices for one block per CU -- every slice fewer is 2 x M x N x 4 bytes of fp32 partials less through HBM and a longer K loop
    // per prologue / epilogue.  Like the single chain above this changes the fp32 summation order with the batch, not the value; the strict mode
    // keeps the rule's slice count.  (Not a launch yet: the rules below see the smaller count.)
    if (!sw.strict_splitk && minb > 0 && q.N % 320 == 0) q.splitk = few_slices(tile256_blocks(q.M, q.N, 1, sw), q.splitk, minb);
    // 3. K-sliced launches small enough to be resident at once fold their slices inside a ping-pong launch (sw.red bit 1).
    if (plan_pp_fold(mode, q, sw, fold_buffer_available, &pl)) return pl;
    // 4. The 256-row tile where it fills the chip: 320 / 256 / 128 wide from big_min_blocks blocks, or -- small batches: 256 x 320 tiles would leave
    // CUs without a block, 256 x 160 tiles (ping-pong loop only) still cover them -- 160 wide from half as many.
    const bool narrow = minb > 0 && sw.pp && q.splitk <= 1 && q.N % 320 == 0 && q.M >= 64 && tile256_blocks(q.M, q.N, 1, sw) < minb &&
                        2 * tile256_blocks(q.M, q.N, 1, sw) >= minb;
    if (narrow || (minb > 0 && tile256_blocks(q.M, q.N, q.splitk, sw) >= minb)) {
        GemmParams c = q;
        c.tile_n = narrow ? 160 : 0;
        if (plan_tile256(mode, c, sw, &pl)) return pl;
    }
    // 5. (round 6) launches too small for either rule above but with a LONG K loop per block: the ping-pong 256 x 160 tile with half the blocks of the
    // 128-row kernel still wins -- its K step costs ~0.45 us per 32 columns against ~1.6 us per 64 for a 128-row block that runs alone on its CU
    // (profiles/r06_gemm_lab_ablation.txt), and the fixed costs of a launch stop mattering.  Zero123++'s CFG pair on a 120 x 80 latent lives here
    // (75-300 blocks of 128 x 160 per conv, K = 2 880 .. 11 520 unsplit or in 2 slices).  Bit-identical like every tile choice.
    if (sw.pp && sw.pp160_min_k > 0 && q.N % 160 == 0 && q.M >= 128 && q.K / gemm_slices(q) >= sw.pp160_min_k) {
        GemmParams c = q;
        c.tile_n = 160;
        if (pp_takes(mode, c, sw, false, &epi)) return plan_of(GEMM_PP, pp_bn(c), 256, GEMM_RING_PINGPONG, epi, c);
    }
    // 6. Everything else: the 128-row kernel.
    return plan_v128(q, sw, fold_buffer_available);
}

// The parameter copy a plan implies: what the kernel of the plan is launched with (`sk_sync`: the fold counters, used when the plan folds).
inline GemmParams gemm_plan_params(const GemmParams& p, const GemmPlan& pl, const GemmSwitches& sw, int* sk_sync) {
    GemmParams q = p;
    q.splitk = pl.splitk;
    q.splitk_seq = pl.splitk_seq;
    q.sk_sync = pl.epilogue == GEMM_EPI_RED ? sk_sync : nullptr;
    if (pl.family == GEMM_PP || pl.family == GEMM_PP2) {
        q.tile_n = pl.tile_n == 160 ? 160 : 0;
        q.old_swizzle = sw.old_swizzle;
        q.dbg = sw.pp_dbg;
    }
    return q;
}

}  // namespace

// The launchers of the 256-row kernels (gemm_big.hip, gemm_pp.hip): `plan` is a GemmPlan of their family, `params` the GemmParams copy it implies
// (gemm_plan_params) -- untyped because both structs have internal linkage.  They launch exactly what the plan names and re-check nothing: a plan
// they have no kernel for is an internal error (MVE_ERR_STATE), not a fallback.  The caller runs the split-K reducer where the plan has one.
int mve_gemm_big_launch(int dtype, int mode, const void* plan, const void* params, void* stream);
int mve_gemm_pp_launch(int dtype, int mode, const void* plan, const void* params, void* stream);
