/*
 * libmvedit_amd — C ABI of the MI355X (gfx950) engine for MVEdit's
 * denoise -> render -> reconstruct hot path.
 *
 * Conventions
 *   - every pointer named d_* (or documented "device") is a device pointer
 *     owned by the CALLER (PyTorch-ROCm storage in the reference host); the
 *     engine never frees or retains caller memory past the call;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all
 *     work is stream-ordered, no call synchronises the device unless its
 *     comment says so;
 *   - return value: 0 on success, negative mve_status on failure;
 *     mve_last_error() returns a thread-local message for the last failure;
 *   - tensors are dense and contiguous in the layout written next to them.
 *
 * Each entry cites the reference interface it replaces (file:line relative to
 * the Lakonik/MVEdit tree).
 */
#ifndef MVEDIT_AMD_H
#define MVEDIT_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVE_API __attribute__((visibility("default")))

typedef enum {
    MVE_OK = 0,
    MVE_ERR_ARG = -1,     /* bad argument / unsupported shape */
    MVE_ERR_HIP = -2,     /* HIP runtime error (message has the hipError string) */
    MVE_ERR_STATE = -3,   /* object used in the wrong state (e.g. weights missing) */
    MVE_ERR_NOMEM = -4    /* caller-provided workspace / capacity too small */
} mve_status;

typedef enum {
    MVE_F32 = 0,
    MVE_F16 = 1,
    MVE_BF16 = 2,
    MVE_I32 = 3,
    MVE_U8 = 4
} mve_dtype;

MVE_API const char* mve_last_error(void);
MVE_API int mve_version(void);                 /* ABI version, bumped on breaking change (library housekeeping: no reference counterpart) */
MVE_API int mve_device_info(int* n_cu, int* wave_size, char* arch, int arch_len); /* hipGetDeviceProperties of the current device */

/* =========================================================================
 * 1. Ray marching (replaces lib/ops/raymarching: bindings.cpp:5-19, kernels
 *    in src/raymarching.cu).  All floating point is fp32 as in the reference
 *    (raymarching.py:33 `custom_fwd(cast_inputs=torch.float32)`).
 * ========================================================================= */

/* raymarching.cu:92-145 kernel_near_far_from_aabb.
 * rays_o, rays_d: [N,3] f32; aabb: [6] f32 device (xmin,ymin,zmin,xmax,ymax,zmax);
 * nears, fars: [N] f32 out.  Miss -> both FLT_MAX. */
MVE_API int mve_near_far_from_aabb(const float* d_rays_o, const float* d_rays_d, const float* d_aabb,
                                   uint32_t N, float min_near, float* d_nears, float* d_fars, void* stream);

/* raymarching.cu:214-226 / :237-254.  coords: [N,3] i32, indices: [N] i32. Bit exact. */
MVE_API int mve_morton3d(const int32_t* d_coords, uint32_t N, int32_t* d_indices, void* stream);
MVE_API int mve_morton3d_invert(const int32_t* d_indices, uint32_t N, int32_t* d_coords, void* stream);

/* raymarching.cu:268-289 kernel_packbits.  grid: [n_bytes*8] f32, bitfield: [n_bytes] u8;
 * bit i of byte n = (grid[8n+i] >= density_thresh). */
MVE_API int mve_packbits(const float* d_grid, uint32_t n_bytes, float density_thresh, uint8_t* d_bitfield, void* stream);

/* raymarching.cu:303-319 kernel_flatten_rays.  rays: [N,2] i32 (offset,count); res: [M] i32 */
MVE_API int mve_flatten_rays(const int32_t* d_rays, uint32_t N, uint32_t M, int32_t* d_res, void* stream);

/* Training-mode march (raymarching.cu:338-475, two passes in the reference with a host
 * read of the atomic counter between them, raymarching.py:285-296).
 *
 * Here the two passes are separate stream-ordered calls and the atomicAdd is replaced by a
 * deterministic exclusive prefix sum in ray order, so rays[n] = (sum_{m<n} count[m], count[n]).
 * (The reference's offsets depend on atomic arrival order; any sequential execution of its
 * threads in ray order yields exactly these values.)
 *
 *  _count : pass 1.  Writes rays[N,2] i32 and d_total[0] = M (i32).  d_scratch: >= mve_march_scratch_bytes(N) bytes.
 *  _write : pass 2.  Writes xyzs[M,3], dirs[M,3], ts[M,2] for rays whose (offset+count) <= capacity;
 *           samples past `capacity` rows are dropped (never written).
 */
MVE_API size_t mve_march_scratch_bytes(uint32_t N);
MVE_API int mve_march_rays_train_count(const float* d_rays_o, const float* d_rays_d, const uint8_t* d_grid,
                                       float bound, int contract, float dt_gamma, uint32_t max_steps,
                                       uint32_t N, uint32_t C, uint32_t H,
                                       const float* d_nears, const float* d_fars, const float* d_noises,
                                       int32_t* d_rays, int32_t* d_total, void* d_scratch, void* stream);
MVE_API int mve_march_rays_train_write(const float* d_rays_o, const float* d_rays_d, const uint8_t* d_grid,
                                       float bound, int contract, float dt_gamma, uint32_t max_steps,
                                       uint32_t N, uint32_t C, uint32_t H,
                                       const float* d_nears, const float* d_fars, const float* d_noises,
                                       const int32_t* d_rays, uint32_t capacity,
                                       float* d_xyzs, float* d_dirs, float* d_ts, void* stream);

/* Capacity form of the training iteration: no host read between the passes.  The caller sizes the sample tensors by a CAPACITY it
 * chooses; how many samples are live is a count in device memory that every following `_n` entry point reads.  None of the `_n` entry
 * points (nor the calls they share kernels with) allocates, copies synchronously or synchronises, so the host never waits inside an
 * iteration.  With any count in [0, capacity], and with a marched total above the capacity, no kernel touches memory outside the
 * capacity-sized buffers: an overflow is a flag, never a fault.  (Bounds rules: mvedit_amd/csrc/capacity_core.h.)
 *
 *  _clamp : runs between _count and _write.  d_n_samples[0] = *d_total, the marched total, also when it exceeds the capacity (so a
 *           caller can size a retry); *d_count = d_n_samples[1] = the samples of the longest prefix of whole rays that fit the
 *           capacity (= the total when nothing overflows); *d_overflow = 1 when total > capacity, otherwise it is left as it is
 *           (sticky: the caller zeroes it).  d_total may alias d_n_samples.  _write, given the same capacity, skips the rays that do
 *           not fit, and so do the composite kernels given M = capacity; rows at and beyond the count are whatever the caller put
 *           there (zeros). */
MVE_API int mve_march_rays_train_clamp(const int32_t* d_rays, uint32_t N, const int32_t* d_total, uint32_t capacity,
                                       int32_t* d_n_samples, int32_t* d_count, int32_t* d_overflow, void* stream);

/* raymarching.cu:501-579 / :606-695.  sigmas[M], rgbs[M,3], ts[M,2], rays[N,2];
 * weights[M] must be zero-initialised by the caller (raymarching.py:330). */
MVE_API int mve_composite_rays_train_forward(const float* d_sigmas, const float* d_rgbs, const float* d_ts,
                                             const int32_t* d_rays, uint32_t M, uint32_t N, float T_thresh, int binarize,
                                             float* d_weights, float* d_weights_sum, float* d_depth, float* d_image,
                                             void* stream);
MVE_API int mve_composite_rays_train_backward(const float* d_grad_weights, const float* d_grad_weights_sum,
                                              const float* d_grad_depth, const float* d_grad_image,
                                              const float* d_sigmas, const float* d_rgbs, const float* d_ts,
                                              const int32_t* d_rays, const float* d_weights_sum, const float* d_depth,
                                              const float* d_image, uint32_t M, uint32_t N, float T_thresh, int binarize,
                                              float* d_grad_sigmas, float* d_grad_rgbs, void* stream);

/* Inference march / composite (raymarching.cu:714-829 / :843-925).
 * xyzs, dirs: [n_alive*n_step,3]; ts: [n_alive*n_step,2] -- must be zeroed by the caller
 * (raymarching.py:428-430: a zero ts[.,0] marks "no sample").  composite mutates
 * rays_alive / rays_t / weights_sum / depth / image in place. */
MVE_API int mve_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t* d_rays_alive, const float* d_rays_t,
                           const float* d_rays_o, const float* d_rays_d, float bound, int contract, float dt_gamma,
                           uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t* d_grid,
                           const float* d_nears, const float* d_fars,
                           float* d_xyzs, float* d_dirs, float* d_ts, const float* d_noises, void* stream);
MVE_API int mve_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int binarize,
                               int32_t* d_rays_alive, float* d_rays_t, const float* d_sigmas, const float* d_rgbs,
                               const float* d_ts, float* d_weights_sum, float* d_depth, float* d_image, void* stream);

/* Stream-ordered compaction of the alive list (replaces the boolean-mask indexing
 * `rays_alive[rays_alive >= 0]`, base_volume_renderer.py:322).  Order preserving.
 * d_n_out[0] = number kept.  d_scratch: >= mve_march_scratch_bytes(n_alive). */
MVE_API int mve_compact_alive(const int32_t* d_rays_alive, uint32_t n_alive, int32_t* d_out, int32_t* d_n_out,
                              void* d_scratch, void* stream);

/* Train branch of VolumeRenderer.forward (lib/models/decoders/base_volume_renderer.py:222-243): keep the samples whose
 * composited weight exceeds `threshold`, order preserving, and re-index rays[N][2] = (offset, count) accordingly.
 * d_pref [M+1] receives the reference's `filt_inds` (exclusive prefix count of kept samples, pref[M] = total kept);
 * d_n_out (device int32) the number kept; outputs are caller-allocated with room for M samples. */
MVE_API size_t mve_cull_scratch_bytes(uint32_t M);
MVE_API int mve_cull_samples(const float* d_weights, uint32_t M, float threshold, const int32_t* d_rays, uint32_t N,
                             const float* d_xyzs, const float* d_dirs, const float* d_ts, float* d_out_xyzs, float* d_out_dirs,
                             float* d_out_ts, int32_t* d_out_rays, int32_t* d_pref, int32_t* d_n_out, void* d_scratch,
                             void* stream);
/* Capacity form: the input count is read from the device (*d_count live rows of `capacity`), the kept count is written to *d_n_out
 * (a different address).  Outputs and d_pref [capacity + 1] are capacity-sized; output rows at and beyond the kept count are zeros.
 * A ray with offset + count above the live count did not fit: it becomes (kept count, 0), and d_pref is never read past the live count.
 * For rays that fit, d_out_rays and the kept count equal mve_cull_samples(M = count).  d_scratch: mve_cull_scratch_bytes(capacity). */
MVE_API int mve_cull_samples_n(const float* d_weights, uint32_t capacity, const int32_t* d_count, float threshold, const int32_t* d_rays,
                               uint32_t N, const float* d_xyzs, const float* d_dirs, const float* d_ts, float* d_out_xyzs,
                               float* d_out_dirs, float* d_out_ts, int32_t* d_out_rays, int32_t* d_pref, int32_t* d_n_out,
                               void* d_scratch, void* stream);

/* Density-grid refresh, the device part of update_extra_state (base_volume_renderer.py:105-177).
 *   density_grid_points : cell coords [N,3] int32 (NULL = every cell of the grid in meshgrid order) + uniform noise [N,3] in
 *                         [0,1) (NULL = cell centres) -> Morton indices [N] and query points
 *                         (coords - (H-1)/2) * 2*bound/H + noise*2*hw - hw,  hw = bound/H   (:129-135)
 *   density_grid_update : tmp[indices] = min(sigmas, FLT_MAX); grid = where(grid >= 0 & tmp >= 0, max(grid*decay, tmp), grid);
 *                         *d_mean = mean(clamp(grid, 0))  (:166-171).  tmp_grid must be pre-filled with -1 by the caller. */
MVE_API int mve_density_grid_points(const int32_t* d_coords, const float* d_noise, uint32_t N, uint32_t grid_size, float bound,
                                    float* d_xyzs, int32_t* d_indices, void* stream);
MVE_API size_t mve_density_grid_scratch_bytes(uint32_t n_cells);
MVE_API int mve_density_grid_update(float* d_density_grid, float* d_tmp_grid, uint32_t n_cells, const float* d_sigmas,
                                    const int32_t* d_indices, uint32_t N, float decay, float* d_mean_density, void* d_scratch,
                                    void* stream);

/* =========================================================================
 * 2. UNet primitives (activations are NHWC = [B*H*W, C] row-major, 16-bit
 *    storage `dtype` in {MVE_F16, MVE_BF16}, fp32 accumulation everywhere).
 *    They replace the third-party arithmetic (diffusers==0.27.2 on cuDNN /
 *    cuBLAS / SDPA) that the reference drives from
 *    lib/models/architecture/diffusers.py:57-164 (unet_enc/unet_dec) and
 *    lib/models/architecture/ip_adapter/attention_processor.py:198-270.
 * ========================================================================= */

#define MVE_GEMM_GEGLU   1   /* W rows interleaved (value,gate): out[m][i] = v[2i]*gelu(v[2i+1]), out width N/2 */
#define MVE_GEMM_OUT_F32 2   /* out is float32 instead of `dtype` */
#define MVE_CONV_W_CHUNK64 4 /* conv weight is [Cout][Cin/64][3][3][64] (needs C1, C2 multiples of 64) */
#define MVE_GEMM_NO_SPLITK 8 /* never split K even if a workspace is given */
#define MVE_CONV_PAD_BR 32    /* stride-2 conv padded on the bottom / right only: diffusers Downsample2D(padding=0) = F.pad(x, (0,1,0,1)) + conv */
#define MVE_GEMM_RES_AFTER_SCALE 16   /* out = (acc + bias) * out_scale + residual (default: residual is added before the scale) */

/* Every Linear / 1x1 Conv2d of the UNet (diffusers Attention, FeedForward, ResnetBlock2D shortcut, Transformer2DModel proj_in/out,
 * TimestepEmbedding; reached through lib/models/architecture/diffusers.py:69-97, :124-162 and the vendored processors,
 * lib/models/architecture/ip_adapter/attention_processor.py:236-262) with its bias / residual / GEGLU epilogue fused:
 * out[m][n] = out_scale * ( sum_k A[m][k]*W[n][k] + bias[n] + rowvec[m/rows_per_vec][n] + residual[m][n] )
 * A: [M][lda] dtype, W: [N][ldw] dtype (torch Linear / 1x1-conv layout; ldw > K selects a column block),
 * out: [M][ldc]; bias: [N] f32 or NULL; rowvec: [ceil(M/rows_per_vec)][ldrv] f32 or NULL (the per-image time
 * embedding of ResnetBlock2D); residual: [M][ldr] dtype or NULL.  N, K, lda, ldw, ldr multiples of 8. */
MVE_API int mve_gemm(int dtype, const void* d_A, int lda, const void* d_W, int ldw, void* d_out, int ldc,
                     int M, int N, int K, const float* d_bias, const float* d_rowvec, int ldrv, int rows_per_vec,
                     const void* d_residual, int ldr, int flags, float out_scale, void* d_workspace,
                     size_t workspace_bytes, int rows_per_image, void* stream);

/* Tuning knob: GEMM / conv launches whose 256 x 320 tiling yields at least `big_min_blocks` (bits 0..24) blocks use the 256-row tile
 * (bit-identical results, so the choice never affects parity or batch invariance).  0 disables it, a negative value only queries.
 * Bit 27 set: the 256-row tile runs the two-stage main loop (csrc/gemm_big.hip) instead of the ping-pong loop (csrc/gemm_pp.hip);
 * bit 30 set (MVE_GEMM_STRICT_SPLITK=1): a launch that fills the chip un-split emulates the K slices of the slice rule inside one block
 * (bitwise equal to split-K + reducer, i.e. to the same rows in a small batch) instead of accumulating K in one chain (the default since
 * round 4: same value up to fp32 summation order, 3.8 ms per 68 ms step faster); bit 29 set: real split-K + reducer there; the two-blocks-per-CU 256 x 160 three-slot tile for dense
 * GEMMs: by default where the dispatcher asks for the narrow tile (launches too small to fill the chip with 320-wide tiles), bit 26 set:
 * wherever it is eligible, bit 28 set: never; bit 25 set: round 2's LDS ring swizzle (A/B aid).  Returns the WHOLE previous word
 * (threshold and option bits), so `old = tune(x); ...; tune(old)` restores every switch.  The defaults come from the environment
 * variables MVE_GEMM_BIG, MVE_GEMM_PP, MVE_GEMM_PP2 (0 never / 1 wherever eligible / 2 narrow launches only) and MVE_GEMM_STRICT_SPLITK. */
MVE_API int mve_gemm_tune(int big_min_blocks);
/* In-kernel K-slice reduction (round 6): a K-sliced GEMM / conv launch that the 256-row ping-pong tile takes folds its slices inside the launch
 * (the blocks of an output tile write their fp32 partial tiles, meet at a per-tile counter, and each folds its share of the tile's rows over the
 * slices in slice order and runs the fused epilogue) instead of leaving them to a second `k_splitk_reduce` launch; small launches (few images per
 * rank) thereby run on the ping-pong loop instead of the 128-row two-stage kernel.  Same slices, same fold order, same epilogue: bit-identical to
 * partials + reducer.  1 (default, MVE_GEMM_RED) on, 0 off, negative only queries.  Returns the previous value. */
MVE_API int mve_gemm_red_tune(int on);
/* The 128-row GEMM / conv kernel with a four-stage LDS ring (k_gemm_deep, csrc/gemm.hip; round 6): launches of at most `max_blocks` blocks -- the
 * K-sliced GEMMs / convs of the deep UNet levels when a rank holds few images, where a block's K loop is a chain of memory round trips -- keep three K
 * tiles in flight instead of one.  Same tile, MFMA order and epilogue as the two-stage loop: bit-identical.  Default 512 (MVE_GEMM_DEEP); 0 turns it
 * off; negative only queries.  Returns the previous value. */
MVE_API int mve_gemm_deep_tune(int max_blocks);
/* Diagnostics: the number of K slices a GEMM / conv launch of this shape runs with under the current switches -- the slice rule's count (a function
 * of rows per image, N, K only), 1 where the un-split launch fills the chip (or the rule's count again in the strict mode, which emulates the slices
 * inside one block), or the smallest count that fills the chip where the rule would over-fill it.  Host logic only. */
MVE_API int mve_gemm_effective_splitk(int M, int N, int K, int rows_per_image);
/* Diagnostics: the dispatch plan of a launch under the current switches (csrc/gemm_dispatch.h: gemm_plan -- the function the entry points launch
 * from).  Host logic only: no GPU is touched, no buffer is needed.  The parameters are filled by the code the entry points use:
 *   kind 0: mve_gemm / mve_gemm_pair / mve_gemm_pair_ln of M x N x K with dense leading dimensions (conv_geom may be null);
 *   kind 1: mve_conv3x3* with conv_geom = {C1, C2, C3, C4, B, Hs, Ws, stride, upsample} and N = Cout (C3 > 0: the shortcut forms); M, K ignored;
 *   kind 2: one launch of mve_upsample_conv_phases with conv_geom = {C, 0, 0, 0, B, Hs, Ws} and N = Cout; M, K ignored.
 * `flags`: the MVE_GEMM_* / MVE_CONV_* flags of the call.  `features`: which optional operands the call has (MVE_PLAN_*).  With MVE_GEMM_RED on,
 * the slice-fold counters are taken to be available.  out[MVE_PLAN_DESCRIBE_INTS] = {family (0: 128-row kernel, 1: 256-row two-stage loop,
 * 2: ping-pong loop, 3: ping-pong three-slot 256 x 160 tile), tile width, tile rows, ring (0: two-stage, 1: four-stage, 2: ping-pong), epilogue
 * (0: plain, 1: residual pair, 2: in-launch slice fold, 3: fused LayerNorm, 4: in-block slice emulation), splitk, splitk_seq, 1 if a split-K
 * reducer launch follows, w_major, grid (blocks), number of such launches the entry point makes (4 for unfused phases), M of the launch}. */
#define MVE_PLAN_RESIDUAL 1
#define MVE_PLAN_RESIDUAL_LO 2
#define MVE_PLAN_OUT_LO 4
#define MVE_PLAN_ROWVEC 8
#define MVE_PLAN_LN 16          /* mve_gemm_pair_ln */
#define MVE_PLAN_BIAS 32
#define MVE_PLAN_WORKSPACE 64   /* a split-K workspace of sufficient size */
#define MVE_PLAN_SCALED 128     /* out_scale != 1 */
#define MVE_PLAN_DESCRIBE_INTS 12
MVE_API int mve_gemm_plan_describe(int kind, int M, int N, int K, int rows_per_image, int flags, int features, const int* conv_geom, int* out);

/* Development aid for csrc/gemm_pp.hip: with `d_buf` (device, 64 uint64 per launched block) set, fp16 320-wide launches of the
 * ping-pong kernel run an instrumented copy and every wave writes its shader-clock sums {L-section work, wait at the L barrier,
 * M-section work, wait at the M barrier, fragment reads, address prep, 0, 0}; NULL turns it off.  (No reference counterpart.) */
MVE_API int mve_gemm_pp_profile(void* d_buf);

/* (No reference counterpart: scheduling detail of mve_gemm / mve_conv3x3.)  Split-K: at the deep UNet levels one image contributes only a few output tiles while K = 9*1280..9*2560; K is then cut
 * into slices that run concurrently and are summed in a fixed order by a second launch.  The slice count depends on
 * (rows_per_image, N, K) only -- never on the batch -- so results are bit-identical however views are chunked or
 * partitioned across GPUs.  It needs an fp32 scratch of mve_gemm_workspace_bytes(...) bytes (0 = this shape never
 * splits; conv: M = B*Ho*Wo, K = 9*(C1+C2), rows_per_image = Ho*Wo); d_workspace NULL or rows_per_image 0 = no split. */
MVE_API size_t mve_gemm_workspace_bytes(int M, int N, int K, int rows_per_image);

/* 3x3 convolution, padding 1, as an implicit GEMM over NHWC input(s):
 *   input = concat_channels(x1[B,Hs,Ws,C1], x2[B,Hs,Ws,C2]) (C2 = 0: single input), optionally
 *   nearest-upsampled 2x (`upsample`; diffusers Upsample2D) and/or strided (`stride` 1|2; Downsample2D);
 *   W: [Cout][3][3][C1+C2] dtype, or with MVE_CONV_W_CHUNK64 [Cout][(C1+C2)/64][3][3][64] (the K order that
 *   keeps the nine taps of a 64-channel slab adjacent; preferred whenever the channel counts allow it);
 *   out: [B*Ho*Wo][ldc]; epilogue as mve_gemm with rows_per_vec = Ho*Wo. */
MVE_API int mve_conv3x3(int dtype, const void* d_x1, int C1, const void* d_x2, int C2, int B, int Hs, int Ws,
                        int stride, int upsample, const void* d_W, int Cout, void* d_out, int ldc,
                        const float* d_bias, const float* d_rowvec, int ldrv, const void* d_residual, int ldr,
                        int flags, float out_scale, void* d_workspace, size_t workspace_bytes, void* stream);

/* ResnetBlock2D tail in one launch: out = conv3x3(x1; W[:, :9*C1]) + conv1x1([x3 | x4]; W[:, 9*C1:]) + bias + bias2 (+ residual).
 * The 1x1 `conv_shortcut` of a resnet whose input and output widths differ (diffusers ResnetBlock2D, reached through
 * lib/models/architecture/diffusers.py:86-97, :139-156) is appended to the K loop of conv2: W is [Cout][9*C1 + C3 + C4] with the 3x3
 * part in MVE_CONV_W_CHUNK64 order followed by the shortcut matrix; x3 / x4 are the (optionally concatenated) block inputs, NHWC
 * at the output resolution.  C1, C3, C4 multiples of 64.  Split-K sizing: mve_gemm_workspace_bytes(M, Cout, 9*C1 + C3 + C4, H*W). */
MVE_API int mve_conv3x3_shortcut(int dtype, const void* x1, int C1, const void* x3, int C3, const void* x4, int C4, int B, int Hs,
                                 int Ws, const void* W, int Cout, void* out, int ldc, const float* bias, const float* bias2,
                                 const void* residual, int ldr, int flags, float out_scale, void* d_workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- nearest-2x upsample + 3 x 3 conv as four 2 x 2 phase convs (round 4) -------------------------------------------------------------------------
 * Replaces, for Upsample2D (diffusers 0.27.2 resnet/upsampling: F.interpolate(scale_factor=2, mode="nearest") then conv 3x3 pad 1; the UNet's
 * up_blocks.*.upsamplers.0 and the VAE decoder's, reached from lib/models/architecture/diffusers.py:57-164 / lib/pipelines/utils.py decode), the
 * fused form mve_conv3x3(..., upsample = 1): output pixel (2 i + py, 2 j + px) reads source rows {i - 1 + py, i + py} and columns
 * {j - 1 + px, j + px} only, the 3 x 3 taps landing on one source pixel add up, so each output parity (py, px) is a 2 x 2 conv over the SOURCE
 * with K = 4 C: 4 / 9 of the multiply-adds.  Zero padding of the upsampled image = zero padding of the source: exact at the borders.
 *   d_W4 : [phase = 2 py + px][Cout][C / 64][2][2][64], the summed taps from mve_pack_upsample_phase_weights (fp32 sums in ascending (row, column)
 *          order, ONE rounding to the storage type).  That rounding is the only arithmetic difference from the 3 x 3 form: the two agree to the
 *          storage precision of the weights, not bit for bit (tests/test_unet_ops.py pins both the exact identity on the rounded phase weights and
 *          the distance to the 3 x 3 form; end to end: tests/rounding_budget_experiment.py --phase).
 *   d_out: [B][2 Hs][2 Ws][Cout] NHWC, dense; d_out_lo (NULL or the same shape in BYTES): the 8-bit low half (lo8, below) in residual_pair mode; needs Cout % 320 == 0.
 * Needs C % 64 == 0, Cout a multiple of 128, Ws a power of two, B Hs Ws >= 64 (mve_upsample_conv_phases_supported = 1); one launch of the
 * ping-pong kernel (2 x 2 window, grouped output rows) for the four phases where B Hs Ws is a multiple of 256, four launches otherwise; K slices by
 * the conv slice rule with 4 Hs Ws rows per image -- batch independent (workspace: *_workspace_bytes). */
MVE_API int mve_upsample_conv_phases_supported(int C, int Cout, int B, int Hs, int Ws);
/* Where B Hs Ws is a multiple of 256 the four phases run as ONE launch of 4 B Hs Ws rows (the phases share the chip like the tiles of any conv: 64
 * images at the 8 x 8 level = one block per CU in one accumulation chain instead of 4 x (64 tiles x 4 K slices + reducer)); same arithmetic per
 * element up to the K-slice policy.  mve_upsample_conv_phases_tune(0): always four launches (A/B; env MVE_PHASES_ONE_LAUNCH); negative: query;
 * returns the previous value. */
MVE_API int mve_upsample_conv_phases_tune(int one_launch);
MVE_API size_t mve_upsample_conv_phases_workspace_bytes(int C, int Cout, int B, int Hs, int Ws);
MVE_API int mve_pack_upsample_phase_weights(int src_dtype, int dst_dtype, const void* d_w_oihw, int Cout, int C, void* d_W4, void* stream);
MVE_API int mve_upsample_conv_phases(int dtype, const void* d_x, int C, int B, int Hs, int Ws, const void* d_W4, int Cout, void* d_out,
                                     const float* d_bias, int flags, void* d_workspace, size_t workspace_bytes, void* d_out_lo, void* stream);

/* ---- residual stream as an unrounded pair (the executor's `residual_pair` mode, mve_unet_set_residual_mode; round 4, the UNet's DEFAULT since round 5) ----
 * The reference's half-precision modules round the residual stream x + f(x) of ResnetBlock2D / BasicTransformerBlock / Transformer2DModel
 * (diffusers 0.27.2, driven from lib/models/architecture/diffusers.py:57-164) to 16 bits after every block: ~30 % of the end-to-end error against
 * fp32 arithmetic (tests/rounding_budget_experiment.py).  In pair mode a stream tensor is stored as hi = round16(x) -- what every MFMA operand
 * read sees, in the tensor's usual place -- and an 8-BIT low half in a companion tensor of the same shape, one byte per element:
 *   lo8 = E5M2( 2^8 * (x - hi) )   (round to nearest even; OCP E5M2 = torch.float8_e5m2; x ~= hi + 2^-8 * lo8, ~14 mantissa bits for fp16 storage).
 * Round 4 kept the low half in 16 bits; 8 bits lose nothing that the end-to-end error can see (8.6e-4 vs 8.7e-4 from fp32 arithmetic at the
 * benchmark shape, 1.23e-3 without a low half) and halve its HBM traffic.  The *_pair entry points are the plain ones plus the companions:
 *   d_residual_lo : lo8 of the residual ([M][ldr] BYTES, NULL = the residual is `d_residual` alone); needs a residual added before the scale;
 *   d_out_lo      : receives lo8(v - round16(v)) next to d_out = round16(v) ([M][ldc] BYTES, NULL = not wanted); 16-bit non-GEGLU outputs only;
 *   d_x*_lo       : lo8 of the normalised inputs (NULL = the input is the 16-bit tensor alone); statistics and the normalisation use hi + lo.
 * With both companions NULL every *_pair call IS the plain call.  A pair launch that is not K-sliced starts its accumulators from the residual
 * pair -- residual + sum_k a w, then + bias -- on EVERY tile the dispatcher may pick (round 5: the 128-row kernel too), so pair launches are
 * bit-identical across tiles exactly as plain launches are (tests/test_unet_ops.py::test_pair_launches_round_identically_on_every_tile); a
 * K-sliced launch adds the pair in the reducer. */
MVE_API int mve_gemm_pair(int dtype, const void* d_A, int lda, const void* d_W, int ldw, void* d_out, int ldc,
                          int M, int N, int K, const float* d_bias, const float* d_rowvec, int ldrv, int rows_per_vec,
                          const void* d_residual, int ldr, int flags, float out_scale, void* d_workspace,
                          size_t workspace_bytes, int rows_per_image, const void* d_residual_lo, void* d_out_lo, void* stream);

/* mve_gemm_pair (no per-image row vector, no GEGLU, unit scale) followed by LayerNorm of the output rows over the N columns:
 *   d_ln_out[m][:] = LayerNorm(row m of the output as a consumer reads it back: hi + lo8 when d_out_lo is given) * gamma + beta   (eps inside the sqrt).
 * Where the launch runs on the 320-wide pair tile (N = 320, M a multiple of 256, bias, no K slices: the residual-stream GEMMs of the 64 x 64 level
 * from 16 images up) the tile that produces a row normalises it in its epilogue -- the row never returns from HBM for its LayerNorm; every other
 * launch is followed by the LayerNorm kernel.  One row arithmetic for both (csrc/ln_core.h): bit-identical results, so the choice may follow the
 * launch geometry.  BasicTransformerBlock norm1 / norm2 / norm3 behind Transformer2DModel.proj_in / attn1.to_out / attn2.to_out (diffusers 0.27.2 as
 * driven from lib/models/architecture/diffusers.py:69-97).  MVE_GEMM_LN_FUSE=0 / mve_gemm_ln_fuse_tune(0): always the separate kernel. */
MVE_API int mve_gemm_pair_ln(int dtype, const void* d_A, int lda, const void* d_W, int ldw, void* d_out, int ldc, int M, int N, int K,
                             const float* d_bias, const void* d_residual, int ldr, void* d_workspace, size_t workspace_bytes, int rows_per_image,
                             const void* d_residual_lo, void* d_out_lo, void* d_ln_out, int ld_ln, const float* d_ln_gamma, const float* d_ln_beta,
                             float ln_eps, void* stream);
MVE_API int mve_gemm_ln_fuse_tune(int on);

MVE_API int mve_conv3x3_pair(int dtype, const void* x1, int C1, const void* x2, int C2, int B, int Hs, int Ws, int stride,
                             int upsample, const void* W, int Cout, void* out, int ldc, const float* bias, const float* rowvec,
                             int ldrv, const void* residual, int ldr, int flags, float out_scale, void* d_workspace,
                             size_t workspace_bytes, const void* d_residual_lo, void* d_out_lo, void* stream);
MVE_API int mve_conv3x3_shortcut_pair(int dtype, const void* x1, int C1, const void* x3, int C3, const void* x4, int C4, int B, int Hs,
                                      int Ws, const void* W, int Cout, void* out, int ldc, const float* bias, const float* bias2,
                                      int flags, float out_scale, void* d_workspace, size_t workspace_bytes, void* d_out_lo, void* stream);
MVE_API int mve_groupnorm_silu_pair(int dtype, const void* d_x1, int C1, const void* d_x2, int C2, int B, int HW, int G,
                                    float eps, const float* d_gamma, const float* d_beta, int silu, void* d_out,
                                    void* d_workspace, const void* d_x1_lo, const void* d_x2_lo, void* stream);
MVE_API int mve_layernorm_pair(int dtype, const void* d_x, int ldx, void* d_y, int ldy, int M, int C,
                               const float* d_gamma, const float* d_beta, float eps, const void* d_x_lo, void* stream);
/* (hi, lo8) = pair of ((a_hi + a_lo) + alpha * b): the ControlNet residual added to a skip tensor of the stream (diffusers.py:110-121); the low halves
 * are lo8 bytes; an all-zero addend leaves the pair untouched bit for bit */
MVE_API int mve_axpy_pair(int dtype, const void* d_a, const void* d_a_lo, const void* d_b, float alpha, void* d_y, void* d_y_lo, size_t n, void* stream);

/* ---- 2b. MXFP8 block-scaled linear (csrc/mxfp8.hip; mvedit_amd/mxfp8.py) ---------------------------------------------------------------------------
 * An 8-bit matrix path on gfx950's block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4), the only instruction that reaches the fp8 rate.  A
 * primitive: no engine uses it yet.  (No reference counterpart: the reference has no fp8)
 *
 * Packed format (OCP MX): a [R][K] matrix, K % 32 == 0, is two byte tensors
 *   q : uint8 [R][Kp], row-major, Kp = 128 * ceil(K / 128) = mve_mxfp8_packed_k(K): OCP e4m3fn bytes (what torch.float8_e4m3fn holds);
 *   e : uint8 [R][Kp / 32], row-major: E8M0 bytes, byte b = 2^(b - 127);
 *   element (r, k) = e4m3(q[r][k]) * 2^(e[r][k / 32] - 127).  Columns K .. Kp-1 are padding: q = 0x00, e = 127 (mve_mxfp8_quantize writes it).
 * Scale rule, per block of 32 consecutive k, on exponents only:
 *   amax = max |x| over the block in fp32; s = the smallest integer with amax * 2^-s <= 448 (amax = m * 2^ex, 0.5 <= m < 1: s = ex - 9 if
 *   m <= 0.875, else ex - 8), clamped to [-127, 127]; amax == 0 gives s = 0; e = s + 127;
 *   q = RNE_e4m3(clamp(x * 2^-s, -448, 448)), the scaling exact (an exponent change).
 *   This is the CLIPPING-FREE variant of the MX rule: the OCP text takes s = floor(log2 amax) - 8 and saturates the elements that then exceed 448;
 *   here the block maximum always fits, at the cost of one bit less for blocks with m > 0.875.  Away from the exponent clamp
 *   |dequantised - x| <= max(2^-4 |x|, 2^-10 * 2^s).
 * Non-finite inputs are outside the contract.  What the kernel does: NaN -> 0 (as the lo8 packer); +-Inf sets its block's scale to s = 120, its
 * own element to +-448, and the block's finite elements are scaled by 2^-120.
 * Host converters with the same bits: mvedit_amd.mxfp8.quantize_host / dequantize_host. */
MVE_API int mve_mxfp8_packed_k(int K);      /* host only: Kp, or -1 when K is not a positive multiple of 32 */
/* d_x: [R][ldx] of `dtype` in {MVE_F32, MVE_F16, MVE_BF16} (ldx >= K in elements: row-strided views), d_q: [R][Kp] 16-byte aligned, d_e: [R][Kp/32]
 * 4-byte aligned.  One pass; 16-byte loads when d_x and its rows are 16-byte aligned, element loads otherwise (same bytes out). */
MVE_API int mve_mxfp8_quantize(int dtype, const void* d_x, int ldx, int R, int K, uint8_t* d_q, uint8_t* d_e, void* stream);
/* out[m][n] = round_once( sum_k A[m][k] * W[n][k] + bias[n] + residual[m][n] ): packed A [M][Kp] / W [N][Kp] (torch Linear layout), fp32
 * accumulation, then (acc + bias) + residual in fp32, one rounding to out_dtype in {MVE_F32, MVE_F16, MVE_BF16}.  d_out: [M][ldc];
 * d_bias: [N] f32 (16-byte aligned) or NULL; d_residual: [M][ldr] of out_dtype or NULL.
 * Constraints: K % 32 == 0, N % 8 == 0, M >= 1, ldc >= N, ldr >= N, d_aq / d_wq 16-byte and d_ae / d_we 4-byte aligned; anything else returns
 * MVE_ERR_ARG with a message that names the argument, before the device is touched.
 * Every output element is ONE fp32 accumulation chain over the 128-wide K steps in ascending order (no K split, no atomics), whatever M and N:
 * two runs give the same bits, and a row's result does not depend on the rows around it. */
MVE_API int mve_mxfp8_gemm(const uint8_t* d_aq, const uint8_t* d_ae, const uint8_t* d_wq, const uint8_t* d_we, int M, int N, int K, int out_dtype,
                           void* d_out, int ldc, const float* d_bias, const void* d_residual, int ldr, void* stream);

/* Scaled-dot-product attention over packed projections (no head permutes):
 *   Q row (b,i) at d_Q + (b*Lq+i)*ldq, head h at column h*head_dim; same for K/V with Lk, O with Lq.
 *   Optional second KV segment (K2,V2,Lk2) is logically concatenated after the first along the key
 *   axis (reference attention: lib/pipelines/zero123plus.py:66-69, lib/models/architecture/diffusers.py:646-673).
 *   Cross-image attention (lib/models/architecture/joint_attn.py:13-17) is B/=n, Lq*=n by the caller.
 *   head_dim in {40, 64, 80, 160}.  Replaces F.scaled_dot_product_attention
 *   (lib/models/architecture/ip_adapter/attention_processor.py:246-248). */
MVE_API int mve_attention(int dtype, const void* d_Q, int ldq, const void* d_K, int ldk, const void* d_V, int ldv,
                          const void* d_K2, int ldk2, const void* d_V2, int ldv2, void* d_O, int ldo,
                          int B, int Lq, int Lk, int Lk2, int heads, int head_dim, float scale, void* stream);
/* Experiment knob (no reference counterpart): 0 = the measured kernel configuration; 1 = for head_dim 40 with a single KV segment, 16
 * query rows per wave, 64-key fills and 3-4 waves per SIMD (the d = 40 case is VALU / exp bound at 2 waves per SIMD).  Results of the
 * two variants agree to rounding, not bitwise (the online-softmax rescale points differ); 2 = for head_dim 80 / 160 a K-tile chunk
 * permutation whose fragment reads are free of LDS bank conflicts (same arithmetic: bit-identical results); 4 = a V^T-tile swizzle
 * that also spreads the transposing stores over the LDS banks (single KV segment, any head_dim; bit-identical results); 6 = 2 + 4;
 * 8..11 = for head_dim 40 the kernel with 32x32x16 Q K^T, LDS-DMA-staged row-major V read through the LDS transpose read and
 * v_permlane16_swap for P (8: 4 waves / 2 LDS stages, 9: 8 waves / 2, 10: 4 waves / 3, 11: 8 waves / 3 stages); other head dims keep 0.
 * Negative: query only.  Returns the previous value (MVE_ERR_ARG for values >= 256 in a release build).  tools/ab_attention.py measures them on one box. */
MVE_API int mve_attention_tune(int variant);
/* Development aid (tools/ab_attention_ablate.py), DEVELOPMENT BUILDS ONLY (MVE_ATTN_LAB=1 python -m mvedit_amd.build): bits 8-19 of
 * mve_attention_tune's argument select a timing-only ablation of the head_dim 40 kernel (results are wrong by construction); those launches add
 * per-wave shader-clock and 100 MHz durations to a device accumulator which this call reads into out4 = {shader cycles, 10 ns ticks, waves, 0}
 * and resets.  A release build carries none of those kernels: this call returns MVE_ERR_STATE and mve_attention_tune rejects the bits. */
MVE_API int mve_attention_profile(unsigned long long* out4);
/* The same attention with Q ALREADY multiplied by softmax_scale * log2(e) (= head_dim^-1/2 * 1.442695...): the logits are in log2 units
 * and no per-logit multiply remains.  This is how the UNet / ControlNet executors call it: they fold the factor into the to_q rows when the
 * weights are packed (fp32 multiply, then the one rounding to 16 bit), which replaces the `scale=` handling of
 * F.scaled_dot_product_attention in the reference's processors (lib/models/architecture/ip_adapter/attention_processor.py:246-248,
 * :348-350, :364-366).  For head_dim 40 and variants 8..11 the running maximum is subtracted by the first MFMA of Q K^T itself. */
MVE_API int mve_attention_prescaled(int dtype, const void* d_Q, int ldq, const void* d_K, int ldk, const void* d_V, int ldv,
                                    const void* d_K2, int ldk2, const void* d_V2, int ldv2, void* d_O, int ldo,
                                    int B, int Lq, int Lk, int Lk2, int heads, int head_dim, void* stream);

/* ---- 2c. CLIP text tower primitives (csrc/clip_text.hip): the arithmetic of transformers' CLIPTextModel / CLIPTextModelWithProjection
 * (models/clip/modeling_clip.py) that the reference's pipelines run as `self.text_encoder` through diffusers' `_encode_prompt`
 * (lib/pipelines/mvedit_3d_pipeline.py:368; the SDXL towers are built at lib/pipelines/utils.py:244-283).  Every argument error returns
 * MVE_ERR_ARG with a message that names the argument, before the device is touched. */

/* Causal scaled-dot-product SELF-attention over packed projections, as mve_attention lays them out (row (b,i) at d_X + (b*L+i)*ldx, head h at
 * column h*64): key j is visible to query i only when j <= i -- the `is_causal=True` attention of CLIPAttention under CLIPTextModel
 * (create_causal_mask + eager / sdpa attention, modeling_clip.py:298-335, :543-556).  head_dim == 64 (ViT-L, OpenCLIP-H and bigG text towers),
 * 1 <= L <= 128 (CLIP: 77); ldq / ldk / ldv multiples of 8 and the three pointers 16-byte aligned.  Logits, mask, maximum, exp and sum in fp32;
 * the causal triangle and the padded tail of the last tile are masked by a select (a masked key takes no part in the maximum and has probability
 * exactly 0; no infinity is formed); fp32 accumulation, one rounding of the output.  One block per (batch item, head): two runs give the same
 * bits, an item's output does not depend on B, and rows <= p do not depend on K / V rows > p. */
MVE_API int mve_attention_causal(int dtype, const void* d_Q, int ldq, const void* d_K, int ldk, const void* d_V, int ldv, void* d_O, int ldo,
                                 int B, int L, int heads, int head_dim, float scale, void* stream);
/* CLIPTextEmbeddings (modeling_clip.py:221-277) with the default position ids: out[b,i,:] = round_once(float(tok[ids[b,i]]) + float(pos[i])).
 * d_ids int32 [B,L]; d_tok [vocab,C], d_pos [max_pos,C] and d_out [B,L,C] in `dtype`, 16-byte aligned; C % 8 == 0; L <= max_pos.  The caller
 * validates the ids; the kernel clamps one outside [0, vocab) so that it cannot read outside the table. */
MVE_API int mve_clip_embed(int dtype, const int32_t* d_ids, const void* d_tok, const void* d_pos, void* d_out, int B, int L, int C, int vocab,
                           int max_pos, void* stream);
/* Elementwise activation in fp32, in or out of place (d_y may equal d_x): CLIPMLP.activation_fn (modeling_clip.py:338-350).
 * MVE_ACT_QUICK_GELU: x * sigmoid(1.702 x) (transformers QuickGELUActivation, `hidden_act='quick_gelu'`); MVE_ACT_GELU: the erf form
 * 0.5 x (1 + erf(x / sqrt 2)) (`hidden_act='gelu'`, nn.GELU()). */
#define MVE_ACT_QUICK_GELU 0
#define MVE_ACT_GELU 1
MVE_API int mve_act(int dtype, int kind, const void* d_x, void* d_y, size_t n, void* stream);
/* The pooled output of CLIPTextModel (modeling_clip.py:561-581): out[b,:] = x[b, pos(b), :] with pos chosen on the device from d_ids int32 [B,L]:
 * eos_token_id == 2 (configs from before transformers PR #24773): the first position of the maximum id; otherwise the first position whose id
 * equals eos_token_id, position 0 when there is none.  d_x [B,L,C], d_out [B,C] in `dtype`. */
MVE_API int mve_clip_pool(int dtype, const void* d_x, const int32_t* d_ids, void* d_out, int B, int L, int C, int eos_token_id, void* stream);

/* ---- 2d. CLIP vision tower primitives (csrc/clip_vision.hip): the arithmetic of transformers' CLIPVisionEmbeddings (models/clip/modeling_clip.py)
 * under `IPAdapter.image_encoder` (lib/models/architecture/ip_adapter/ip_adapter.py:51-53, :130, :138), `Zero123PlusPipeline.vision_encoder`
 * (lib/pipelines/zero123plus.py:372) and `Zero123Pipeline.image_encoder` (lib/pipelines/zero123.py:260).  `dtype` is f16 or bf16, pointers are
 * 16-byte aligned; every argument error returns MVE_ERR_ARG with a message that names the argument, before the device is touched. */

/* The operand rows of `patch_embedding` = Conv2d(3, C, kernel = stride = P, bias=False) as a GEMM: with G = H / P, row b*G*G + gy*G + gx of
 * d_rows [B*G*G][ld] holds the patch (gy, gx) of image b in (channel, ky, kx) order -- the order of weight.reshape(C, 3*P*P) -- and the columns
 * from 3*P*P up to ld = 8 * ceil(3*P*P / 8) are zero (mve_gemm wants K % 8 == 0: patch 14 gives 588 -> 592).  d_pixels [B,3,H,W] NCHW.
 * Pure data movement, no arithmetic.  H % P == 0, W == H. */
MVE_API int mve_clip_patchify(int dtype, const void* d_pixels, int B, int H, int W, int P, void* d_rows, int ld, void* stream);
/* CLIPVisionEmbeddings' sum: out[b,0,:] = round_once(float(cls) + float(pos[0])), out[b,1+p,:] = round_once(float(patch[b,p]) + float(pos[1+p])).
 * d_patch [B*G2][C], d_cls [C], d_pos [G2+1][C], d_out [B][G2+1][C]; C % 8 == 0. */
MVE_API int mve_clip_vision_embed(int dtype, const void* d_patch, const void* d_cls, const void* d_pos, void* d_out, int B, int G2, int C, void* stream);

/* ---- 2e. DPT-hybrid primitives (csrc/dpt.hip): the row kernels of the Omnidata normal predictor, the reference's
 * `DPTDepthModel(backbone='vitb_rn50_384', num_channels=3)` (omnidata_modules/midas/dpt_depth.py:87-107, loaded at lib/apis/adapter3d.py:338-352,
 * called through `enable_normals`, lib/pipelines/mvedit_3d_pipeline.py:262-273), that the GEMM / conv / norm / attention primitives do not give.
 * Activations NHWC, `dtype` f16 or bf16, C % 8 == 0, pointers 16-byte aligned; every argument error returns MVE_ERR_ARG before the device is
 * touched. */

/* The operand rows of the ResNetV2 stem: Conv2d(3, C, 7, stride 2) with TF "same" padding of an even image (2 before, 3 after) as a GEMM.
 * Row (b*Ho + oy)*Ho + ox (Ho = S / 2) of d_rows [B*Ho*Ho][ld] holds pixels[b][c][2 oy - 2 + ky][2 ox - 2 + kx] in (c, ky, kx) order -- the order
 * of weight.reshape(C, 147) -- zero outside the image; columns 147 .. ld - 1 are zero.  ld must be 152.  d_pixels [B,3,S,S] NCHW.  No arithmetic. */
MVE_API int mve_dpt_stem_rows(int dtype, const void* d_pixels, int B, int S, void* d_rows, int ld, void* stream);
/* Max-pool 3 x 3 / 2 with "same" padding of an even map (0 before, 1 after; taps outside the map are left out): x [B,H,W,C] -> y [B,H/2,W/2,C].
 * transformers pads with 0, timm with -inf; behind a ReLU (x >= 0) they agree, and this kernel agrees with both.  Exact. */
MVE_API int mve_dpt_maxpool(int dtype, const void* d_x, int B, int H, int W, int C, void* d_y, void* stream);
/* y[b, oy, ox, :] = x[b, 2 oy, 2 ox, :]: the operand rows of a stride-2 1 x 1 convolution (the downsample shortcut).  H, W even.  Exact. */
MVE_API int mve_dpt_gather_s2(int dtype, const void* d_x, int B, int H, int W, int C, void* d_y, void* stream);
/* F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True): x [B,H,W,C] -> y [B,2H,2W,C], torch's fp32 arithmetic (source coordinate
 * dst * (H-1)/(2H-1)), one rounding to `dtype`. */
MVE_API int mve_dpt_upsample2x(int dtype, const void* d_x, int B, int H, int W, int C, void* d_y, void* stream);
/* y = max(a + b, 0) elementwise, the sum in fp32, one rounding; d_b NULL: y = max(a, 0).  In place allowed (d_y == d_a).  n % 8 == 0. */
MVE_API int mve_dpt_add_relu(int dtype, const void* d_a, const void* d_b, void* d_y, size_t n, void* stream);

/* ---- 2f. LoFTR matcher primitives (csrc/loftr.hip): the kernels of the reference's detector-free feature matcher (loftr/, loaded at
 * lib/apis/adapter3d.py:411-415, run once per Zero123++ view by lib/core/utils/pose_estimation.py:30-160) that the GEMM / conv / norm primitives do
 * not give.  16-bit activations are `dtype` f16 or bf16 with C % 8 == 0 and 16-byte aligned pointers; similarity, confidence, statistics, key
 * points and expectations are fp32; match ids are int64 (what the reference's callers index with).  Every reduction is fp32 in a fixed order (no
 * float atomics): two runs give identical bits.  Every argument error returns MVE_ERR_ARG before the device is touched. */

/* The operand rows of the stem Conv2d(1, C, 7, stride 2, padding 3) as a GEMM: row (b*Ho + oy)*Wo + ox (Ho = H/2, Wo = W/2) of d_rows [B*Ho*Wo][ld]
 * holds pixels[b][0][2 oy - 3 + ky][2 ox - 3 + kx] at column ky*7 + kx -- the order of weight.reshape(C, 49) -- zero outside the image; columns
 * 49 .. 55 are zero.  ld must be 56.  d_pixels [B,1,H,W], H and W even.  No arithmetic. */
MVE_API int mve_loftr_stem_rows(int dtype, const void* d_pixels, int B, int H, int W, void* d_rows, int ld, void* stream);
/* y = x (x >= 0), slope * x (x < 0), the product in fp32, one rounding (the FPN heads' LeakyReLU).  In place allowed.  n % 8 == 0. */
MVE_API int mve_loftr_leaky_relu(int dtype, const void* d_x, void* d_y, size_t n, float slope, void* stream);
/* y[b, p, :] = round_once(float(x[b, p, :]) + pos[p, :]): d_x, d_y [B][HW][C], d_pos fp32 [HW][C] (the sinusoidal table, built by the caller). */
MVE_API int mve_loftr_pos_add(int dtype, const void* d_x, const float* d_pos, void* d_y, int B, int HW, int C, void* stream);

/* Linear attention ("Transformers are RNNs") with phi(x) = elu(x) + 1 taken in fp32 from the 16-bit operand, in two steps.
 *   mve_linattn_kv:    d_kv[(b*H + h)][0 .. D*D)   = KV[d][v] = sum_s phi(K[b,s,h,d]) V[b,s,h,v]   (row-major [D][D])
 *                      d_kv[(b*H + h)][D*D .. +D)  = Ksum[d]  = sum_s phi(K[b,s,h,d])
 *   mve_linattn_apply: out[b,l,h,:] = phi(Q[b,l,h,:]) . KV / (phi(Q[b,l,h,:]) . Ksum + eps), rounded once to `dtype`.
 * K, V [B][S][ld], Q, out [B][L][ld]; head h occupies columns [h*D, (h+1)*D); D is 32 or 16; ld % 8 == 0.  d_kv fp32 [B*H][D*D + D].
 * fp32 accumulators: S is cut into 128-row chunks, one block each, every thread sums its rows in ascending order and the chunk partials are
 * added in ascending order (d_workspace >= mve_linattn_workspace_bytes; 0 for S <= 128).  The reference's division of V by S and
 * multiplication back -- a guard against fp16 overflow, the identity in exact arithmetic -- is left out. */
MVE_API size_t mve_linattn_workspace_bytes(int B, int S, int H, int D);
MVE_API int mve_linattn_kv(int dtype, const void* d_k, int ldk, const void* d_v, int ldv, int B, int S, int H, int D, float* d_kv, void* d_workspace,
                           size_t workspace_bytes, void* stream);
MVE_API int mve_linattn_apply(int dtype, const void* d_q, int ldq, const float* d_kv, void* d_out, int ldo, int B, int L, int H, int D, float eps,
                              void* stream);

/* Dual softmax of a similarity d_sim fp32 [N][L][ld]; only columns [0, S) are read (ld > S: the padding of a GEMM's leading dimension).
 *   mve_dsmax_stats: d_row_stats [N*L][2] = (max_j, sum_j exp(sim - max)), d_col_stats [N*S][2] = (max_i, sum_i exp(sim - max)).
 *   mve_dsmax_conf:  d_conf fp32 [N][L][S] (compact) = softmax over i  *  softmax over j -- the reference's `conf_matrix`. */
MVE_API int mve_dsmax_stats(const float* d_sim, int N, int L, int S, int ld, float* d_row_stats, float* d_col_stats, void* stream);
MVE_API int mve_dsmax_conf(const float* d_sim, int N, int L, int S, int ld, const float* d_row_stats, const float* d_col_stats, float* d_conf, void* stream);
/* Mutual-nearest selection (get_coarse_match without masks): cell i = y0*W0 + x0 of pair n matches j = y1*W1 + x1 when conf[n][i][j] > thr, every
 * one of y0, x0, y1, x1 is at least `border` cells from both edges of its grid (border <= 0: no rule), and conf[n][i][j] equals the maximum of its
 * row and of its column; of several such j (exactly equal floats) the lowest.  Survivors are compacted in ascending (n, i) order: d_b_ids / d_i_ids /
 * d_j_ids int64 and d_mconf fp32 with room for N * L entries, d_count int32 [1] (device).  d_mkpts0_c / d_mkpts1_c (fp32 [N*L][2], may be NULL)
 * receive (x, y) * scale.  d_conf [N][H0*W0][H1*W1] compact; d_workspace >= mve_dsmax_select_workspace_bytes(N, L, S). */
MVE_API size_t mve_dsmax_select_workspace_bytes(int N, int L, int S);
MVE_API int mve_dsmax_select(const float* d_conf, int N, int H0, int W0, int H1, int W1, float thr, int border, float scale, int64_t* d_b_ids,
                             int64_t* d_i_ids, int64_t* d_j_ids, float* d_mconf, float* d_mkpts0_c, float* d_mkpts1_c, int* d_count, void* d_workspace,
                             size_t workspace_bytes, void* stream);

/* F.unfold(feat, 5, stride 4, padding 2) at the matched coarse cells only: d_rows[(m*25 + ky*5 + kx)][:] = feat[b_ids[m]][4 cy - 2 + ky][4 cx - 2 + kx][:],
 * (cy, cx) = (ids[m] / (Wf/4), ids[m] % (Wf/4)), zero outside the map (and for an id outside its range).  d_feat [N][Hf][Wf][C] NHWC, Hf and Wf
 * multiples of 4; d_b_ids / d_ids int64 [M] on the device; M >= 1 is a host value.  Exact. */
MVE_API int mve_loftr_unfold(int dtype, const void* d_feat, int N, int Hf, int Wf, int C, const int64_t* d_b_ids, const int64_t* d_ids, int M, void* d_rows,
                             void* stream);
/* y[m, :] = x[m, :] + LayerNorm(o[m, :]) * gamma + beta (LoFTREncoderLayer's `x + norm2(message)`), fp32 throughout, one rounding; y may alias x.
 * o [M][ldo], x [M][ldx], y [M][ldy]; C a multiple of 64, at most 512; gamma / beta fp32 [C]. */
MVE_API int mve_loftr_ln_add(int dtype, const void* d_o, int ldo, const void* d_x, int ldx, void* d_y, int ldy, int M, int C, const float* d_gamma,
                             const float* d_beta, float eps, void* stream);
/* d_rows[m, :] = feat[b_ids[m]][ids[m]][:] (zero for an id outside its range): the coarse features at the matched cells.  d_feat [N][L][C]. */
MVE_API int mve_loftr_gather_rows(int dtype, const void* d_feat, int N, int L, int C, const int64_t* d_b_ids, const int64_t* d_ids, int M, void* d_rows,
                                  void* stream);
/* FineMatching: for match m the centre row (12) of window 0 against the 25 rows of window 1 (d_feat0 / d_feat1 [M][25][C]), softmax at 1/sqrt(C),
 * expectation over the normalised 5 x 5 grid in [-1, 1] (x fastest), all in fp32:
 *   d_expec_f [M][3] = (E[x], E[y], sqrt(max(Var x, 1e-10)) + sqrt(max(Var y, 1e-10))),  d_mkpts1_f [M][2] = d_mkpts1_c[m] + (E[x], E[y]) * radius
 * (radius = (window / 2) * image size / fine map size, in pixels). */
MVE_API int mve_loftr_fine_match(int dtype, const void* d_feat0, const void* d_feat1, int M, int C, const float* d_mkpts1_c, float radius, float* d_expec_f,
                                 float* d_mkpts1_f, void* stream);

/* ---- 2g. Segment Anything image encoder primitives (csrc/sam.hip): what segment_anything's `ImageEncoderViT` (the same arithmetic as
 * transformers' SamVisionEncoder, models/sam/modeling_sam.py) has and the primitives above do not give.  The reference reaches it through
 * `SamPredictor.set_image` (lib/apis/adapter3d.py:363-372, :723-734; lib/pipelines/utils.py:114-131).  `dtype` is f16 or bf16, C % 8 == 0,
 * pointers are 16-byte aligned; every argument error returns MVE_ERR_ARG with a message that names the argument, before the device is touched. */

/* Self-attention with MViTv2's decomposed relative-position bias over packed projections, laid out as mve_attention's: NS independent sequences
 * of gh x gw tokens, row (s, i) at d_X + (s*gh*gw + i)*ldx, head h at column h*head_dim, token i at grid position (i / gw, i % gw).
 *   O[q] = softmax_k( scale * Q[q].K[k] + Q[q].rel_h[qh - kh + gh - 1] + Q[q].rel_w[qw - kw + gw - 1] ) V[k]
 * d_rel_h [2gh-1][head_dim] and d_rel_w [2gw-1][head_dim] in `dtype`, shared by every sequence and head; the UNSCALED Q multiplies them
 * (SamVisionAttention.get_decomposed_rel_pos with equal query and key grids and tables of exactly 2n-1 rows: no interpolation).
 * head_dim 64 or 80; gh, gw >= 1 and gh + gw <= 128 (the per-query products Q.rel_h^T, Q.rel_w^T are formed once per 64-query tile by MFMA and
 * kept in LDS as fp32, 2 (gh + gw) - 2 values per query: 64 x 64 needs ~100 KB of the CU's 160 KB); ldq / ldk / ldv multiples of 8.  Logits, both bias terms, maximum, exp and sum in
 * fp32 -- the bias is never rounded to 16 bit; the tail of the last 64-key tile is masked by a select (probability exactly 0, no infinity is
 * formed); both products on the MFMA, fp32 accumulation, one rounding of O.  No atomics: two runs give the same bits, and a sequence's result
 * does not depend on NS. */
MVE_API int mve_attention_relpos(int dtype, const void* d_Q, int ldq, const void* d_K, int ldk, const void* d_V, int ldv, const void* d_rel_h,
                                 const void* d_rel_w, void* d_O, int ldo, int NS, int gh, int gw, int heads, int head_dim, float scale, void* stream);
/* SamVisionLayer.window_partition / window_unpartition: d_x [B][G][G][C] <-> d_win [B * nw * nw][window * window][C] with nw = ceil(G / window);
 * window (b, wy, wx) holds the pixels (wy*window + ty, wx*window + tx).  Partition writes ZEROS for the rows of the padded map (bottom and right,
 * up to nw * window) that have no source pixel; un-partition copies the kept rows back and never reads the padded ones.  1 <= window <= G.
 * Pure data movement in 16-byte vectors, no arithmetic. */
MVE_API int mve_sam_window_partition(int dtype, const void* d_x, int B, int G, int C, int window, void* d_win, void* stream);
MVE_API int mve_sam_window_unpartition(int dtype, const void* d_win, int B, int G, int C, int window, void* d_x, void* stream);
/* hidden_states + pos_embed: y[b, p, :] = round_once(float(x[b, p, :]) + float(pos[p, :])); d_x, d_y [B][HW][C], d_pos [HW][C], all in `dtype`.
 * In place allowed (d_y == d_x). */
MVE_API int mve_sam_pos_add(int dtype, const void* d_x, const void* d_pos, void* d_y, int B, int HW, int C, void* stream);

/* ---- 2h. Segment Anything prompt encoder, mask decoder and mask post-processing primitives (csrc/sam_decoder.hip): what `SamPredictor.predict`
 * runs behind the image encoder (lib/apis/adapter3d.py:721-735, lib/pipelines/utils.py:108-146), stated as transformers' SamPromptEncoder /
 * SamMaskDecoder / SamPositionalEmbedding (models/sam/modeling_sam.py; the same arithmetic as segment_anything's).  ALL OF THEM ARE fp32 --
 * parameters, activations and accumulation -- except the two that touch the encoder: mve_sam_preprocess writes its input in the
 * encoder's dtype and mve_sam_src reads its output.  No atomics, no split-K: two runs give the same bits and an item's result does not depend on
 * the number of items in the launch.  Every argument error returns MVE_ERR_ARG before the device is touched. */

/* uint8 image [h][w][3] (already resized: longest side S) -> d_out [1][3][S][S] in `dtype` (f16 | bf16): (x - pixel_mean[c]) / pixel_std[c] in fp32
 * with one rounding; the pad region (rows >= h, columns >= w) is zero in normalised space, as `Sam.preprocess` pads after normalising.
 * pixel_mean / pixel_std: HOST pointers to 3 floats, NULL = segment_anything's 123.675, 116.28, 103.53 / 58.395, 57.12, 57.375. */
MVE_API int mve_sam_preprocess(int dtype, const uint8_t* d_image, int h, int w, int S, const float* pixel_mean, const float* pixel_std, void* d_out, void* stream);
/* The image-wide positional encoding d_out [G*G][C]: cell (i, j) has coordinates ((j + 0.5) / G, (i + 0.5) / G); c = 2 c - 1, c @ d_gaussian
 * [2][C/2], times 2 pi, [sin | cos] with sinf / cosf (SamModel.get_image_wide_positional_embeddings, channels last). */
MVE_API int mve_sam_dense_pe(const float* d_gaussian, float* d_out, int G, int C, void* stream);
/* d_out [N][T][C]: the iou token, the num_mask_tokens mask tokens, then the sparse prompt embeddings -- points first, box corners after.  A
 * point (x, y) of d_points [N][n_points][2] is the positional encoding of ((x + 0.5) / image_size, (y + 0.5) / image_size) plus
 * d_point_embed[label] for label 0 | 1 (d_labels [N][n_points] int32); for label -1 the row is d_not_a_point.  Points without a box
 * (d_boxes NULL) get one padding point of label -1 appended.  The corners (x0, y0), (x1, y1) of d_boxes [N][4] use d_point_embed[2] / [3]
 * (d_point_embed [4][C]).  T must equal 1 + num_mask_tokens + n_points (+ 1 padding point) + 2 (with a box) and be at most 16. */
MVE_API int mve_sam_prompt_tokens(const float* d_boxes, const float* d_points, const int32_t* d_labels, int N, int n_points, const float* d_gaussian,
                                  const float* d_point_embed, const float* d_not_a_point, const float* d_iou_token, const float* d_mask_tokens, int num_mask_tokens,
                                  int C, float image_size, float* d_out, int T, void* stream);
/* d_embedding [B][C][G][G] in `dtype` (NCHW) -> d_out fp32 rows [N * G^2][C]: item n reads image n / P (N = B * P); + d_no_mask_embed[C]. */
MVE_API int mve_sam_src(int dtype, const void* d_embedding, const float* d_no_mask_embed, float* d_out, int N, int P, int C, int G, void* stream);
/* out [M][N] = A [M][K] . W [N][K]^T (+ d_bias [N]) (+ d_res [M][N], row stride ldr) (ReLU when relu != 0), row-major fp32 with row strides lda /
 * ldw / ldc.  Plain VALU FMA over 64 x 64 LDS tiles (gfx950's fp32 MFMA runs at the vector rate).  Per output element: K in steps of 16, the 16
 * products of a step summed in k order into a partial, the partials added in step order -- fixed, and independent of M and of the tile. */
MVE_API int mve_gemm_f32(const float* d_A, int lda, const float* d_W, int ldw, const float* d_bias, const float* d_res, int ldr, float* d_out, int ldc, int M, int N,
                         int K, int relu, void* stream);
/* softmax(scale * Q K^T) V per (item, head) in fp32, operands laid out as mve_attention's: row (b, i) at d_X + (b * L + i) * ldx, head h at column
 * h * head_dim.  head_dim 16 | 32, any Lq, Lk >= 1, row strides multiples of 4, pointers 16-byte aligned.  Lk <= 16: one thread per (item, query,
 * head) and an online softmax over the keys; Lk > 16: one block per (item, query, head), thread t walks keys t, t + 256, ..., the 256 partial
 * (max, sum, acc) triples merged by a tree in a fixed order.  A tail is a guard on the key index; no infinity is formed. */
MVE_API int mve_attention_f32(const float* d_Q, int ldq, const float* d_K, int ldk, const float* d_V, int ldv, float* d_O, int ldo, int NB, int Lq, int Lk,
                              int heads, int head_dim, float scale, void* stream);
/* torch.nn.LayerNorm over the last dimension of dense fp32 rows (two-pass mean / variance, one wave per row); in place allowed. */
MVE_API int mve_layernorm_f32(const float* d_x, float* d_y, int rows, int C, const float* d_gamma, const float* d_beta, float eps, void* stream);
/* y[r, :] = x[r, :] + pe[r mod period_rows, :] over dense fp32 rows (queries + point embedding: period = rows; keys + dense PE: period = G^2). */
MVE_API int mve_add_rows_f32(const float* d_x, const float* d_pe, float* d_y, int rows, int C, int period_rows, void* stream);
/* ConvTranspose2d(Cin, Cout, kernel 2, stride 2) over pixel rows d_x [N * Gi^2][Cin]: a GEMM against d_W4 [4 Cout][Cin] (row (2 ky + kx) Cout + co
 * = weight[ci][co][ky][kx]) into d_tmp [N * Gi^2][4 Cout], then the pixel shuffle to d_out [N][2 Gi][2 Gi][Cout] rows with the bias and what
 * follows the convolution: mode 1 = LayerNorm2d over the channels of a pixel (d_ln_gamma / d_ln_beta, eps) then erf GELU, mode 2 = erf GELU. */
MVE_API int mve_sam_upscale(const float* d_x, const float* d_W4, const float* d_bias, const float* d_ln_gamma, const float* d_ln_beta, float eps, float* d_tmp,
                            float* d_out, int N, int Gi, int Cin, int Cout, int mode, void* stream);
/* The num_mask_tokens hypernetwork MLPs and the iou head in one launch, each proj_in -> ReLU -> layers.0 -> ReLU -> proj_out (no sigmoid).
 * MLP j < num_mask_tokens reads token 1 + j of d_queries [N][T][C] and writes d_hyper [N][num_mask_tokens][out_dim]; MLP num_mask_tokens (the iou
 * head) reads token 0 and writes d_iou [N][num_mask_tokens].  Stacked weights, the iou head last: d_w0 [Mt+1][hidden][C], d_w1
 * [Mt+1][hidden][hidden], d_w2 [Mt+1][out_dim][hidden] (the iou head fills its first Mt rows), biases alike.  Widths at most 512. */
MVE_API int mve_sam_token_mlps(const float* d_queries, int N, int T, int C, int hidden, int out_dim, int num_mask_tokens, const float* d_w0, const float* d_b0,
                               const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2, float* d_hyper, float* d_iou, void* stream);
/* d_low_res [N][Mt][pixels] = sum_c d_hyper [N][Mt][c] * d_up [N][pixels][c], c ascending. */
MVE_API int mve_sam_mask_product(const float* d_hyper, const float* d_up, float* d_low_res, int N, int num_mask_tokens, int Cu, int pixels, void* stream);
/* `Sam.postprocess_masks` + threshold: d_low_res [planes][L][L] resized bilinearly (align_corners = False) to S x S, cropped to [:h_in, :w_in],
 * resized bilinearly to (H, W) -- composed on the fly, 16 low-res reads per output pixel, no S x S buffer -- then d_masks [planes][H][W] uint8 =
 * value > mask_threshold; d_logits (NULL or fp32 of the same shape) receives the value itself.  Bilinear rule as ATen states it:
 * src = max((dst + 0.5) * (in / out) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1), the scale in fp32. */
MVE_API int mve_sam_postprocess(const float* d_low_res, int planes, int L, int S, int h_in, int w_in, int H, int W, float mask_threshold, uint8_t* d_masks,
                                float* d_logits, void* stream);

/* GroupNorm over NHWC input (optionally the channel-concat of two tensors) with optional fused SiLU (`silu` = 1) or ReLU (`silu` = 2):
 *   out[B*HW][C1+C2] = act( (x - mean_g) * rstd_g * gamma + beta ), torch.nn.GroupNorm semantics.
 * gamma/beta: [C1+C2] f32.  d_workspace: >= mve_groupnorm_workspace_bytes(B,HW,C,G) bytes.
 * (ResnetBlock2D.norm1/norm2 + nonlinearity, Transformer2DModel.norm, conv_norm_out of diffusers 0.27.2,
 * reached from lib/models/architecture/diffusers.py:86-97,139-162.) */
/* Tensors of at most `fused_max_hw` pixels per image whose (image, lcm(C / G, 8)-channel chunk) slice fits one block's registers take the
 * one-launch path (statistics and normalisation out of registers: one read + one write); the choice depends on (HW, C, G) only, never on
 * the batch.  Default 1024 (MVE_GN_FUSED_MAX_HW); 0 disables; negative only queries.  Returns the previous value. */
MVE_API int mve_groupnorm_tune(int fused_max_hw);
MVE_API size_t mve_groupnorm_workspace_bytes(int B, int HW, int C, int G);
MVE_API int mve_groupnorm_silu(int dtype, const void* d_x1, int C1, const void* d_x2, int C2, int B, int HW, int G,
                               float eps, const float* d_gamma, const float* d_beta, int silu, void* d_out,
                               void* d_workspace, void* stream);

/* LayerNorm over the last axis of x[M][ldx] (C <= 2048, C % 8 == 0); gamma/beta f32 [C]: BasicTransformerBlock.norm1/2/3 of
 * diffusers 0.27.2, reached through the Transformer2DModel calls at lib/models/architecture/diffusers.py:91-96, :128-133, :150-155. */
MVE_API int mve_layernorm(int dtype, const void* d_x, int ldx, void* d_y, int ldy, int M, int C,
                          const float* d_gamma, const float* d_beta, float eps, void* stream);

/* Boundary helpers: the reference seam `unet(sample, t, ...)` is NCHW (adapter3d_mixin.py:117-125). */
MVE_API int mve_nchw_to_nhwc(int dst_dtype, int src_dtype, const void* d_x, int B, int C, int H, int W, int Cpad,
                             void* d_y, void* stream);
MVE_API int mve_nhwc_to_nchw(int dst_dtype, int src_dtype, const void* d_x, int ld, int B, int C, int H, int W,
                             void* d_y, void* stream);
/* diffusers Timesteps(dim, flip_sin_to_cos=True, downscale_freq_shift=0): out[b] = [cos(t*f_k) | sin(t*f_k)] */
MVE_API int mve_timestep_embedding(int dtype, const float* d_t, int B, int dim, void* d_out, void* stream);
/* The operand row of add_embedding.linear_1 under addition_embed_type='text_time' (diffusers 0.27.2 UNet2DConditionModel.get_aug_embed):
 *   out[b] = cat([text_embeds[b], Timesteps(time_embed_dim, flip_sin_to_cos=True, freq_shift=0)(time_ids[b]).flatten()]).to(dtype)
 * i.e. [B, text_dim + n_ids * time_embed_dim] in `dtype` (f16 | bf16): the converted text_embeds (text_dtype: f32 | f16 | bf16), then per time id
 * time_embed_dim values, cosines first, then sines.  d_time_ids is f32 [B, n_ids]. */
MVE_API int mve_text_time_embedding(int dtype, const void* d_text_embeds, int text_dtype, int text_dim, const float* d_time_ids, int n_ids,
                                    int time_embed_dim, int B, void* d_out, void* stream);
MVE_API int mve_silu(int dtype, const void* d_x, void* d_y, size_t n, void* stream);
MVE_API int mve_axpy(int dtype, const void* d_a, const void* d_b, float alpha, void* d_y, size_t n, void* stream); /* y = a + alpha*b */
/* probs[m][:N] = softmax(scores[m][:N]) (fp32 in, `dtype` out): the softmax of the VAE mid-block attention (diffusers Attention with
 * heads = 1, dim_head = 512, reached through self.vae.decode / .encode, lib/pipelines/mvedit_3d_pipeline.py:1260, :1441), which
 * runs as scores = mve_gemm(Q, K) -> mve_softmax_rows -> mve_gemm(P, V^T). */
MVE_API int mve_softmax_rows(int dtype, const float* d_scores, size_t lds, int M, int N, void* d_probs, size_t ldp, void* stream);
/* classifier-free guidance, adapter3d_mixin.py:130-134: out = g*text + (1-g)*uncond (f32) */
MVE_API int mve_cfg_combine(const float* d_uncond, const float* d_text, float guidance_scale, float* d_out, size_t n,
                            void* stream);
/* x0 = (latents_scaled - sqrt(1-abar_t) * noise_pred) / sqrt(abar_t): `pred_original_sample` of the reference's denoise loop
 * (lib/pipelines/mvedit_3d_pipeline.py:1253-1255), fp32 in / out. */
MVE_API int mve_x0_prediction(const float* d_latents_scaled, const float* d_noise_pred, float sqrt_alpha_bar,
                              float sqrt_one_minus_alpha_bar, size_t n, float* d_x0, void* stream);

/* Tone-mapping look-up table of the pipelines (lib/models/decoders/tonemapping.py:33-54): piecewise-linear interpolation between the
 * `steps` knots (lut_x[k], lut_y[k]) with torch.bucketize(right=True) bucket selection.  inverse = 0: Tonemapping.lut (linear != 0:
 * input_mode='linear', x -> log2(max(x, 1e-6)) first); inverse = 1: Tonemapping.inverse_lut (linear != 0: output_mode='linear',
 * exp2 of the result).  fp32, any shape (n elements); tables are device pointers. */
MVE_API int mve_tonemap_lut(const float* d_x, size_t n, const float* d_lut_x, const float* d_lut_y, int steps, int inverse, int linear,
                            float* d_out, void* stream);
/* Its backward: grad_x = grad_out * d lut / d x (the slope of the selected segment times the derivative of the log2 / exp2 around it) --
 * the reference's lut / inverse_lut are differentiable torch expressions and sit inside the optimisation loops
 * (lib/pipelines/mvedit_3d_pipeline.py:419-420, :438-439, :568-571). */
MVE_API int mve_tonemap_lut_backward(const float* d_x, const float* d_grad_out, size_t n, const float* d_lut_x, const float* d_lut_y,
                                     int steps, int inverse, int linear, float* d_grad_x, void* stream);

/* torchvision.transforms.functional.gaussian_blur on `planes` f32 images [H, W] (reflect padding by ksize / 2, normalised float32 kernel;
 * evaluated separably) as the pipelines use it: target-mask blur (lib/pipelines/mvedit_3d_pipeline.py:473, :671) and `highpass`
 * (lib/pipelines/utils.py:187-188: offset + x - blur(x, 6 round(std) + 1, std), applied to normal patches every iteration, :623-624).
 *   d_base == NULL : out = blur(x)                 d_base != NULL : out = offset + base - blur(x)      (highpass: base = x)
 *   adjoint != 0   : the transposed operator (backward of either form: pass the incoming gradient as x, and as base with offset 0
 *                    for highpass).  tmp: planes * H * W floats, distinct from x and out; out may alias base. */
MVE_API int mve_gaussian_blur(const float* d_x, int planes, int H, int W, int ksize, float sigma, int adjoint, const float* d_base,
                              float offset, float* d_tmp, float* d_out, void* stream);

/* lib/ops/shencoder (src/shencoder.cu:28-337, :359-384; sphere_harmonics.py): real spherical harmonics of inputs [B,3] f32 up to `degree`
 * (1..8) -> outputs [B, degree^2], index l^2 + l + m, Condon-Shortley phase, the un-normalised polynomial form (equal to Y_lm on the unit
 * sphere); dy_dx (nullable) [B, 3, degree^2] = d outputs / d (x, y, z).  Backward: grad_inputs [B,3] = sum_ch grad[b][ch] dy_dx[b][d][ch]
 * (written, not accumulated: the reference's wrapper hands in zeros). */
MVE_API int mve_sh_encode(const float* d_inputs, uint32_t B, int degree, float* d_outputs, float* d_dy_dx, void* stream);
MVE_API int mve_sh_encode_backward(const float* d_grad, const float* d_dy_dx, uint32_t B, int degree, float* d_grad_inputs, void* stream);
/* Shading of a batch of rendered views in one pass (lib/pipelines/mvedit_3d_pipeline.py:1372-1384, same expression at :155-168):
 *   n_cv = (2 n0 - 1, 1 - 2 n1, 1 - 2 n2) from normal_fg;  shading = max(light_v . n_cv, 0) * (1 - ambient) + ambient;
 *   tables given : image = lut(inverse_lut(rgb / max(a, 1e-6)) + log2(max(shading, 1e-6))) * a + bg * (1 - a)
 *   tables NULL  : image = rgb * shading + bg * (1 - a)                                   (`self.tonemapping is None`)
 * rgba [n_views * pix][4], normal_fg [n_views * pix][3], cam_lights [n_views][3], image [n_views * pix][3], all f32. */
MVE_API int mve_shade_views(const float* d_rgba, const float* d_normal_fg, const float* d_cam_lights, uint32_t n_views,
                            uint32_t pix_per_view, float ambient_light, float bg_color, const float* d_lut_x, const float* d_lut_y,
                            int steps, float* d_image, void* stream);
/* Per-point Lambertian shading of the mesh path, forward and backward: the `shading_fun`s handed to MeshRenderer.forward
 * (lib/pipelines/mvedit_3d_pipeline.py:410-440):  shading = max(light_i . normal_i, 0) * (1 - ambient) + ambient;
 *   tables given: out = lut(inverse_lut(albedo) + log2(max(shading, 1e-6)))      tables NULL: out = albedo * shading
 * albedo / normal / lights / out [N,3] f32.  d_grad_out == NULL: forward into d_out.  Otherwise: d_grad_albedo / d_grad_normal [N,3]
 * receive the gradients of <grad_out, out> (d_out may be NULL). */
MVE_API int mve_shade_points(const float* d_albedo, const float* d_normal, const float* d_lights, size_t N, float ambient_light,
                             const float* d_lut_x, const float* d_lut_y, int steps, float* d_out, const float* d_grad_out,
                             float* d_grad_albedo, float* d_grad_normal, void* stream);

/* Image-space loss of one NeRF optimisation iteration and its gradients: lib/pipelines/mvedit_3d_pipeline.py:542-603 (`nerf_optim`,
 * from `out_rgbs = outputs['image']...` to `loss = loss + entropy_loss`) with depth_to_normal (lib/core/utils/geometry_utils.py:119-148),
 * TVLoss(power=1.5) (lib/models/losses/tv_loss.py), L1LossMod (lib/models/losses/pixelwise_loss.py) and Tonemapping.lut / inverse_lut.
 * N = P * ps * ps rays, patch-major ([P, ps, ps] flattened); everything f32, device pointers.
 *   shaded            `not is_init or init_shaded` (:558);  lut_steps = 0 with NULL tables: `self.tonemapping is None`
 *   pixel_loss_weight loss_weight of nerf.pixel_loss (1.2, lib/pipelines/utils.py:231); is_init selects the alpha factor 5 / 1 (:580)
 *   patch_w [P]       cam_weights[target_cam_ids] / cam_weights_mean (`target_w`, constant over a patch, :531-532)
 *   patch_lights [P,3] cam_lights[target_cam_ids] (:533-534)
 *   target_n / target_depth  NULL when `use_normal` / `use_depth` is false
 *   weights [M], ts [M,2]    per-sample outputs of composite_rays_train (entropy term, :596-603); M may be 0 */
typedef struct MveReconLossDesc {
    int32_t P, ps, shaded, is_init, lut_steps;
    float ambient_light, bg_color, normal_bg[3];
    float pixel_loss_weight, normal_reg_weight, depth_weight, entropy_weight, bg_width;
    const float *d_lut_x, *d_lut_y;
    const float *d_image, *d_weights_sum, *d_depth;     /* outputs['image'] [N,3], ['weights_sum'] [N], ['depth'] [N] */
    const float *d_weights, *d_ts;
    uint32_t M;
    const float *d_target_dir, *d_target_rgbs, *d_target_m, *d_target_n, *d_target_depth;   /* [N,3] [N,3] [N] [N,3] [N] */
    const float *d_patch_w, *d_patch_lights;
} MveReconLossDesc;
MVE_API size_t mve_recon_loss_workspace_bytes(int P, int ps, uint32_t M);
/* losses[6] = total (`loss` at :603), pixel_rgb_loss, alphas_loss, normal_reg_loss, depth_loss, entropy_loss; out_rgbs [N,3] and
 * out_normals [N,3] are the tensors the patch (LPIPS) losses of :611-627 consume.  The workspace keeps the normals for the backward. */
MVE_API int mve_recon_loss_forward(const MveReconLossDesc* desc, void* d_ws, size_t ws_bytes, float* d_losses, float* d_out_rgbs,
                                   float* d_out_normals, void* stream);
/* Gradients of g_loss * loss + <g_out_rgbs, out_rgbs> + <g_out_normals, out_normals> (either may be NULL) w.r.t. image [N,3],
 * weights_sum [N], depth [N] and weights [M]: what loss.backward() hands to composite_rays_train's backward.  d_g_loss: one f32 on the
 * device (autograd's incoming gradient, read by the kernels so that the host never waits for it), NULL = 1.  Must follow a forward on
 * the same descriptor and workspace.  Pure gathers: no atomics, bitwise reproducible. */
MVE_API int mve_recon_loss_backward(const MveReconLossDesc* desc, void* d_ws, size_t ws_bytes, const float* d_g_out_rgbs,
                                    const float* d_g_out_normals, const float* d_g_loss, float* d_g_image, float* d_g_weights_sum, float* d_g_depth,
                                    float* d_g_weights, void* stream);
/* Capacity forms: desc->M is the capacity of weights / ts / g_weights (it sizes the workspace), *d_count the live samples.  Only the
 * entropy term sees samples: one at or beyond the count adds nothing to the loss and gets a zero gradient, whatever its row holds.
 * losses, out_rgbs, out_normals and the gradients' live rows equal the exact call on M = count bit for bit. */
MVE_API int mve_recon_loss_forward_n(const MveReconLossDesc* desc, const int32_t* d_count, void* d_ws, size_t ws_bytes, float* d_losses,
                                     float* d_out_rgbs, float* d_out_normals, void* stream);
MVE_API int mve_recon_loss_backward_n(const MveReconLossDesc* desc, const int32_t* d_count, void* d_ws, size_t ws_bytes,
                                      const float* d_g_out_rgbs, const float* d_g_out_normals, const float* d_g_loss, float* d_g_image,
                                      float* d_g_weights_sum, float* d_g_depth, float* d_g_weights, void* stream);

/* The same for one MESH optimisation iteration: lib/pipelines/mvedit_3d_pipeline.py:745-782 (`mesh_optim`, from `out_alphas =
 * render_out['rgba']...` to the regularised sum; the two mesh regularisers of that sum are mve_mesh_reg_*).  N = n * size * size pixels,
 * view-major; rgba [N,4], normal [N,3], depth [N] = render_out['rgba' / 'normal' / 'depth'] (depth only feeds the detached cosine
 * weighting of :751-758), target_m_erode [N] the 5x5-eroded mask (:723-724), view_w [n] = cam_weights / cam_weights_mean. */
typedef struct MveMeshLossDesc {
    int32_t n, size, mesh_is_simplified;
    float normal_bg[3];
    float pixel_loss_weight, normal_reg_weight;
    const float *d_rgba, *d_normal, *d_depth;
    const float *d_target_dir, *d_target_rgbs, *d_target_m_erode, *d_target_m_blur, *d_target_n;   /* [N,3] [N,3] [N] [N] [N,3] or NULL */
    const float *d_view_w;
} MveMeshLossDesc;
MVE_API size_t mve_mesh_loss_workspace_bytes(int n, int size);
/* losses[4] = pixel_rgb_loss + alphas_loss + normal_reg_loss, and the three parts (alpha / normal terms 0 when mesh_is_simplified);
 * out_rgbs [N,3] / out_normals [N,3]: the tensors the patch losses of :784-818 cut their patches from. */
MVE_API int mve_mesh_loss_forward(const MveMeshLossDesc* desc, void* d_ws, size_t ws_bytes, float* d_losses, float* d_out_rgbs,
                                  float* d_out_normals, void* stream);
/* Gradients of g_loss * loss + <g_out_rgbs, out_rgbs> + <g_out_normals, out_normals> w.r.t. rgba [N,4] and normal [N,3] (d_g_loss: one
 * f32 on the device, NULL = 1; the ext gradients may be NULL).  One launch, pure gather. */
MVE_API int mve_mesh_loss_backward(const MveMeshLossDesc* desc, void* d_ws, size_t ws_bytes, const float* d_g_out_rgbs,
                                   const float* d_g_out_normals, const float* d_g_loss, float* d_g_rgba, float* d_g_normal, void* stream);

/* Mesh regularisers of the mesh-optimisation loop and their gradients: laplacian_smooth_loss(verts, faces) and
 * normal_consistency(face_normals, faces) of lib/models/decoders/mesh_renderer/base_mesh_renderer.py:55-101 (with
 * compute_edge_to_face_mapping :20-52 and laplacian_uniform :71-91), called per iteration at lib/pipelines/mvedit_3d_pipeline.py:775-776.
 * verts [V,3] f32, faces [F,3] i32 (indices in [0, V)), face_normals [F,3] f32.  losses[0] = mean_i |(D - A) v|_i over the V vertices
 * (A: distinct neighbours); losses[1] = mean over the unique edges of |1 - clamp(n_t0 . n_t1, -1, 1)| with t0 / t1 the faces listing
 * the edge as (min, max) / (max, min), face 0 where a side is missing (the reference's default).  The workspace carries the per-vertex
 * edge buckets from the forward to the backward. */
MVE_API size_t mve_mesh_reg_workspace_bytes(int V, int F);
MVE_API int mve_mesh_reg_forward(const float* d_verts, int V, const int32_t* d_faces, int F, const float* d_face_normals, void* d_ws,
                                 size_t ws_bytes, float* d_losses, void* stream);
/* g_losses: two f32 on the device (autograd's incoming gradients of the two losses), NULL = (1, 1).  g_verts [V,3] receives the Laplacian
 * term's gradient (normal_consistency does not depend on verts directly), g_face_normals [F,3] the consistency term's. */
MVE_API int mve_mesh_reg_backward(const float* d_verts, int V, const int32_t* d_faces, int F, const float* d_face_normals, void* d_ws,
                                  size_t ws_bytes, const float* d_g_losses, float* d_g_verts, float* d_g_face_normals, void* stream);

/* Mesh.auto_normal (lib/models/decoders/mesh_renderer/mesh_utils.py:359-382, seamless=False; once per mesh-optimisation iteration,
 * lib/pipelines/mvedit_3d_pipeline.py:846-847): face_normals [F,3] = normalize(cross(v1 - v0, v2 - v0)), vn [V,3] = normalize of their
 * per-vertex sum (float atomics, like the reference's scatter_add_).  vn_sum [V,3] (the unnormalised sums) is kept for the backward. */
MVE_API int mve_mesh_normals_forward(const float* d_verts, int V, const int32_t* d_faces, int F, float* d_face_normals, float* d_vn_sum,
                                     float* d_vn, void* stream);
/* g_verts [V,3] = gradient w.r.t. the vertices given g_vn [V,3] and / or g_face_normals [F,3] (either may be NULL); scratch: [V,3] f32. */
MVE_API int mve_mesh_normals_backward(const float* d_verts, int V, const int32_t* d_faces, int F, const float* d_vn_sum, const float* d_g_vn,
                                      const float* d_g_face_normals, float* d_scratch, float* d_g_verts, void* stream);

/* Capacity (host-read-free) form of the four calls above, for a mesh out of mve_dmtet_extract_n (rules: csrc/mesh_capacity_core.h).
 * verts [v_cap,3], faces [f_cap,3]; d_live = device int32 [2] = (live vertices, live faces), clamped into [0, capacity] where it is read.
 * Faces and vertices at or beyond the live counts contribute nothing, are never dereferenced and receive zero gradient; padded rows of
 * face_normals and vn are written as (0, 0, 0) on every call.  The half-edge buckets are built from the live faces only, the means
 * divide by the live counts and the loss tree runs over the live 256-vertex blocks only, in the exact call's order: the two losses
 * equal mve_mesh_reg_forward(V = live vertices, F = live faces) bit for bit.  Zero live faces: both losses and every gradient are 0.
 * Workspace: mve_mesh_reg_workspace_bytes(v_cap, f_cap). */
MVE_API int mve_mesh_reg_forward_n(const float* d_verts, int v_cap, const int32_t* d_faces, int f_cap, const int32_t* d_live,
                                   const float* d_face_normals, void* d_ws, size_t ws_bytes, float* d_losses, void* stream);
MVE_API int mve_mesh_reg_backward_n(const float* d_verts, int v_cap, const int32_t* d_faces, int f_cap, const int32_t* d_live,
                                    const float* d_face_normals, void* d_ws, size_t ws_bytes, const float* d_g_losses, float* d_g_verts,
                                    float* d_g_face_normals, void* stream);
MVE_API int mve_mesh_normals_forward_n(const float* d_verts, int v_cap, const int32_t* d_faces, int f_cap, const int32_t* d_live,
                                       float* d_face_normals, float* d_vn_sum, float* d_vn, void* stream);
MVE_API int mve_mesh_normals_backward_n(const float* d_verts, int v_cap, const int32_t* d_faces, int f_cap, const int32_t* d_live,
                                        const float* d_vn_sum, const float* d_g_vn, const float* d_g_face_normals, float* d_scratch,
                                        float* d_g_verts, void* stream);

/* =========================================================================
 * 3. UNet2DCondition executor (native runtime behind the reference's UNet seam).
 *    Replaces `self.unet(sample, t, encoder_hidden_states=..., cross_attention_kwargs=...,
 *    down_block_additional_residuals=..., mid_block_additional_residual=...)`
 *    (lib/pipelines/adapter3d_mixin.py:117-125) and `unet_enc` / `unet_dec`
 *    (lib/models/architecture/diffusers.py:57-99 / :102-164).
 *
 *    Topology arguments are diffusers' UNet2DConditionModel config values: per level i,
 *    block_out_channels[i], down_attn[i] (CrossAttnDownBlock2D vs DownBlock2D), num_heads[i],
 *    transformer_layers[i].  Weights are engine-owned: mve_unet_load_param copies one tensor of
 *    the diffusers state dict (by its diffusers name, in its torch layout, any float dtype) into
 *    packed device storage; the caller's tensor is not retained.  A name the configuration does
 *    not have, an element count that differs from the parameter's, or a 3 x 3 convolution whose
 *    shape is not exactly [O, I, 3, 3] is refused with MVE_ERR_ARG before the device is touched.
 * ========================================================================= */
MVE_API int mve_unet_create(void** handle, int dtype, int in_channels, int out_channels, int n_levels,
                            const int* block_out_channels, int layers_per_block, const int* down_attn,
                            const int* num_heads, const int* transformer_layers, int cross_attention_dim,
                            int norm_num_groups, float norm_eps, int use_linear_projection);
MVE_API int mve_unet_destroy(void* handle);
MVE_API size_t mve_unet_weight_bytes(void* handle);
MVE_API int mve_unet_load_param(void* handle, const char* name, const void* d_src, int src_dtype, int ndim,
                                const long long* shape, void* stream);
/* returns the number of diffusers parameters not loaded yet; buf receives the first missing name */
MVE_API int mve_unet_missing_params(void* handle, char* buf, int buf_len);

/* (No reference counterpart: executor introspection.)  Builds (and caches) the static op list for this problem size.
 * flops[5] = analytic 2*MAC counts per class {conv3x3, linear/1x1, attention, norm, other}; SURVEY.md section 8(d) quotes their sum.
 * For UNet and ControlNet handles; a handle of another kind is MVE_ERR_ARG (the other engines have their own *_plan). */
MVE_API int mve_unet_plan(void* handle, int B, int H, int W, int ctx_len, int num_cross_attn_imgs, int has_residuals,
                          int io_dtype, int residuals_nhwc, size_t* workspace_bytes, int* n_ops, double* flops);

/* phase 0: full forward; 1: unet_enc only (state stays in the workspace); 2: unet_dec only (same workspace).
 * sample: [B, in_channels, H, W] NCHW io_dtype; timesteps: [B] f32 device; ctx: [B, ctx_len, cross_dim] io_dtype;
 * num_cross_attn_imgs: CrossImageAttnProcWrapper group size (lib/models/architecture/joint_attn.py:11-37), 1 = off;
 * down_residuals: host array of n_levels*(layers_per_block+1) device pointers (ControlNet down_block_res_samples, NCHW io_dtype,
 * or NHWC engine dtype if residuals_nhwc) or NULL; out: [B, out_channels, H, W] NCHW io_dtype.
 * op_ms: optional HOST array [n_ops]; when given every op is bracketed with HIP events on `stream` and the call
 * synchronises the stream before returning (profiling mode). */
MVE_API int mve_unet_forward(void* handle, int phase, const void* d_sample, int io_dtype, const float* d_timesteps,
                             const void* d_ctx, int B, int H, int W, int ctx_len, int num_cross_attn_imgs,
                             const void* const* down_residuals, const void* d_mid_residual, int residuals_nhwc,
                             void* d_out, void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream);
/* ControlNetModel (diffusers; lib/pipelines/adapter3d_mixin.py:101-116, :173-186, :279-287 call it through MultiControlNetModel):
 * the UNet's conv_in + down blocks + mid block, a conditioning embedding on the 8H x 8W control image that is added to
 * conv_in(sample), and one 1x1 "zero" convolution per skip / mid tensor.  Same topology arguments and parameter-loading
 * protocol as the UNet (mve_unet_load_param / _missing_params / _plan / _weight_bytes / _destroy work on the handle; parameter
 * names are the ControlNetModel state-dict names).
 *   d_cond       [B, conditioning_channels, 8H, 8W] NCHW in io_dtype ([B / R, ...] after mve_controlnet_set_cond_repeat(handle, R))
 *   d_outputs    n_levels*(layers_per_block+1) + 1 device pointers: down_block_res_samples then mid_block_res_sample, each NHWC
 *                [B*h*w, C] in the ENGINE dtype -- exactly what mve_unet_forward accepts with residuals_nhwc = 1
 *   out_k = conditioning_scale * zero_conv_k(feature_k), or, with accumulate != 0, out_k += that (MultiControlNetModel's sum) */
MVE_API int mve_controlnet_create(void** handle, int dtype, int in_channels, int conditioning_channels, int n_levels,
                                  const int* block_out_channels, int layers_per_block, const int* down_attn, const int* num_heads,
                                  const int* transformer_layers, int cross_attention_dim, int norm_num_groups, float norm_eps,
                                  int use_linear_projection);
/* Shared conditioning images: with repeat = R >= 1, d_cond of mve_controlnet_forward holds B / R images and batch item b uses image b mod (B / R).
 * Under classifier-free guidance both halves of the batch carry the same control images (lib/pipelines/mvedit_3d_pipeline.py:1232, :1417:
 * `ctrl_images.split(diff_bs) * 2`): the conditioning embedding (8 convs on the 8H x 8W image, ~10 % of a ControlNet forward) then runs once for
 * both.  Bit-identical to passing the images R times.  Part of the plan key; returns the previous value (repeat < 1: query).  Not combined with the
 * residual-pair mode. */
MVE_API int mve_controlnet_set_cond_repeat(void* handle, int repeat);
/* Context tail of a UNet / ControlNet handle (CNAttnProcessor / CNAttnProcessor2_0, lib/models/architecture/ip_adapter/attention_processor.py:400-480:
 * `encoder_hidden_states[:, :end_pos]` with end_pos = L - num_tokens).  Under an IP-Adapter the context is [text rows | image tokens] and the
 * reference's ControlNets cross-attend to the text rows alone.  With rows = n > 0 every later plan / forward of the handle ignores the last n rows
 * of every item's d_ctx: the cross-attention K/V GEMM reads the first ctx_len - n rows of each item (one strided device copy inside the plan, no
 * caller-side copy), bit-identical to passing those rows as a dense [B, ctx_len - n, D] context.  n >= ctx_len is MVE_ERR_ARG at plan time, as is
 * the combination with ip_tokens > 0 (mve_unet_set_attention).  Part of the plan key, and with it of the hipGraph key.  Returns the previous
 * value (rows < 0: query).  A handle that is neither a UNet nor a ControlNet is MVE_ERR_ARG. */
MVE_API int mve_unet_set_context_tail(void* handle, int rows);
MVE_API int mve_controlnet_forward(void* handle, const void* d_sample, int io_dtype, const float* d_timesteps, const void* d_ctx,
                                   const void* d_cond, int B, int H, int W, int ctx_len, float conditioning_scale, int accumulate,
                                   void* const* d_outputs, void* d_workspace, size_t workspace_bytes,
                                   float* op_ms /* optional host array [n_ops]: per-op milliseconds (synchronises) */, void* stream);

/* AutoencoderKL halves (diffusers==0.27.2 autoencoders/vae.py Decoder / Encoder with post_quant_conv / quant_conv), replacing
 *   self.vae.decode(x0 / scaling_factor, return_dict=False)[0]   lib/pipelines/mvedit_3d_pipeline.py:1258-1262, adapter3d_mixin.py:327-338
 *   self.vae.encode(images * 2 - 1, ...)                          lib/pipelines/mvedit_3d_pipeline.py:1118-1120, :1439-1443
 * half 1: [B, in_channels = latent, H, W] -> [B, out_channels, H * 2^(n-1), W * 2^(n-1)];
 * half 2: [B, in_channels = image, H, W] -> [B, out_channels = 2 * latent, H / 2^(n-1), W / 2^(n-1)] = cat(mean, logvar) (the
 *         DiagonalGaussianDistribution arithmetic on those moments stays with the caller).
 * The handle is an executor handle: parameters arrive through mve_unet_load_param under their AutoencoderKL state-dict names
 * (`decoder.*` + `post_quant_conv.*` for half 1, `encoder.*` + `quant_conv.*` for half 2; a name of the other half is an error),
 * mve_unet_missing_params / mve_unet_op_info / mve_unet_destroy apply unchanged.  ResnetBlock2D without time embedding, eps as
 * given (1e-6 in diffusers); mid-block Attention (1 head of width C) = GEMM q k^T (fp32 scores) -> mve_softmax_rows -> GEMM P V;
 * Downsample2D(padding=0) = MVE_CONV_PAD_BR.  in/out channels <= 8.  d_in / d_out are NCHW in io_dtype (f32 | f16 | bf16).
 * One call handles B images whose widest full-resolution activation has < 2^31 elements (8 images at 512 x 512 for the SD VAE). */
MVE_API int mve_vae_create(void** handle, int dtype, int half, int in_channels, int out_channels, int n_levels,
                           const int* block_out_channels, int layers_per_block, int norm_num_groups, float norm_eps);
MVE_API int mve_vae_plan(void* handle, int B, int H, int W, int io_dtype, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_vae_forward(void* handle, const void* d_in, int io_dtype, int B, int H, int W, void* d_out, void* d_workspace,
                            size_t workspace_bytes, float* op_ms, void* stream);

/* SRVGGNetCompact (`image_enhancer` of the pipelines: lib/models/decoders/image_space_ss.py:8-70, built at lib/pipelines/utils.py:212-215
 * with num_feat 64, num_conv 32, upscale 4, PReLU; called on every batch of rendered views below 512 x 512,
 * lib/pipelines/mvedit_3d_pipeline.py:1399-1400).  [B, C, H, W] -> [B, C, H * r, W * r]: conv3x3 + per-channel PReLU stack at the
 * input resolution, conv to C * r * r channels, PixelShuffle(r), plus the nearest-upsampled input.  An executor handle: parameters
 * through mve_unet_load_param under the module's own state-dict names (`body.<i>.weight|bias`), mve_unet_missing_params /
 * mve_unet_op_info / mve_unet_destroy apply.  num_out_ch == num_in_ch <= 8, num_feat % 8 == 0. */
MVE_API int mve_srvgg_create(void** handle, int dtype, int num_in_ch, int num_out_ch, int num_feat, int num_conv, int upscale);
MVE_API int mve_srvgg_plan(void* handle, int B, int H, int W, int io_dtype, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_srvgg_forward(void* handle, const void* d_in, int io_dtype, int B, int H, int W, void* d_out, void* d_workspace,
                              size_t workspace_bytes, float* op_ms, void* stream);
/* CLIP text tower (`text_encoder` / `text_encoder_2` of the pipelines: transformers CLIPTextModel and CLIPTextModelWithProjection,
 * models/clip/modeling_clip.py:494-586, :835-895; built at lib/pipelines/utils.py:244-283 and called through diffusers' `_encode_prompt`,
 * lib/pipelines/mvedit_3d_pipeline.py:368).  An executor handle: parameters through mve_unet_load_param under transformers' own state-dict
 * names (`text_model.embeddings.{token,position}_embedding.weight`, `text_model.encoder.layers.N.{layer_norm1,layer_norm2}.{weight,bias}`,
 * `...self_attn.{q,k,v,out}_proj.{weight,bias}`, `...mlp.{fc1,fc2}.{weight,bias}`, `text_model.final_layer_norm.{weight,bias}`,
 * `text_projection.weight` when projection_dim > 0); mve_unet_missing_params / mve_unet_op_info / mve_unet_destroy apply.
 * Per layer: LayerNorm, one q|k|v GEMM over the packed [3C, C] weight, mve_attention_causal (scale = 64^-1/2), out_proj GEMM + residual,
 * LayerNorm, fc1 GEMM, mve_act, fc2 GEMM + residual; then final LayerNorm, mve_clip_pool, and the bias-free text_projection GEMM.
 * hidden == heads * 64, hidden <= 2048 (mve_layernorm), intermediate % 8 == 0, projection_dim % 8 == 0 (0 = no projection), act in
 * {MVE_ACT_QUICK_GELU, MVE_ACT_GELU}; the forward's eos_token_id selects the pooling rule of mve_clip_pool.  d_ids int32 [B,L], 1 <= L <= min(max_pos, 128),
 * validated by the caller.  Outputs in the handle's dtype: d_last_hidden_state [B,L,C], d_pooler_output [B,C], d_text_embeds [B,P] (required
 * when the handle has a projection, NULL otherwise); d_hidden_states: NULL, or layers + 1 pointers to [B,L,C] tensors that receive the embedding
 * output and every layer's output (before the final norm), transformers' `output_hidden_states=True`. */
MVE_API int mve_clip_text_create(void** handle, int dtype, int vocab_size, int max_position_embeddings, int hidden_size, int num_layers,
                                 int num_heads, int intermediate_size, int act, float layer_norm_eps, int projection_dim);
MVE_API int mve_clip_text_plan(void* handle, int B, int L, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_clip_text_forward(void* handle, const int32_t* d_ids, int B, int L, int eos_token_id, void* d_last_hidden_state,
                                  void* d_pooler_output, void* d_text_embeds, void* const* d_hidden_states, void* d_workspace, size_t workspace_bytes, float* op_ms,
                                  void* stream);
/* CLIP vision tower (transformers CLIPVisionModel / CLIPVisionModelWithProjection; the reference's `IPAdapter.image_encoder`,
 * `Zero123PlusPipeline.vision_encoder`, `Zero123Pipeline.image_encoder`).  An executor handle like the text tower: parameters through
 * mve_unet_load_param under transformers' own names (`vision_model.embeddings.{class_embedding, patch_embedding.weight, position_embedding.weight}`,
 * `vision_model.pre_layrnorm.*` (sic), `vision_model.encoder.layers.N.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.{fc1,fc2}}.*`,
 * `vision_model.post_layernorm.*`, `visual_projection.weight` when projection_dim > 0); the patch weight is stored [C][Kp], zero-padded, at load;
 * mve_unet_missing_params / mve_unet_op_info / mve_unet_destroy apply.
 * Plan: mve_clip_patchify, patch GEMM, mve_clip_vision_embed, pre_layrnorm; per layer LayerNorm, one q|k|v GEMM over the packed [3C, C] weight,
 * mve_attention (Lq = Lk = G*G + 1, scale = head_dim^-1/2), out_proj GEMM + residual, LayerNorm, fc1 GEMM, mve_act, fc2 GEMM + residual; then
 * last_hidden_state = the encoder output WITHOUT post_layernorm (transformers' definition; the text tower's differs), pooler_output =
 * post_layernorm(last_hidden_state[:, 0]) (one mve_layernorm over B rows with ldx = (G*G+1) * C), image_embeds = the bias-free projection GEMM.
 * GEMMs never split K: an item's result does not depend on the batch.
 * Refused at create: hidden / heads not 64 or 80 (OpenCLIP bigG's 104 is refused, not approximated), hidden > 2048 (mve_layernorm),
 * image_size % patch_size != 0, intermediate_size or projection_dim not a multiple of 8 (projection_dim 0 = no projection), act outside
 * {MVE_ACT_QUICK_GELU, MVE_ACT_GELU}.
 * d_pixels [B,3,S,S] NCHW in the handle's dtype, 16-byte aligned.  Outputs in the handle's dtype: d_last_hidden_state [B,G*G+1,C], d_pooler_output
 * [B,C], d_image_embeds [B,P] (required when the handle has a projection, NULL otherwise); d_hidden_states: NULL, or layers + 1 pointers to
 * [B,G*G+1,C] tensors -- entry 0 is the pre_layrnorm output, as in transformers' `output_hidden_states=True`. */
MVE_API int mve_clip_vision_create(void** handle, int dtype, int image_size, int patch_size, int hidden_size, int num_layers, int num_heads,
                                   int intermediate_size, int act, float layer_norm_eps, int projection_dim);
MVE_API int mve_clip_vision_plan(void* handle, int B, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_clip_vision_forward(void* handle, const void* d_pixels, int B, void* d_last_hidden_state, void* d_pooler_output, void* d_image_embeds,
                                    void* const* d_hidden_states, void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream);
/* IP-Adapter "plus" image projection: the reference's Resampler (lib/models/architecture/ip_adapter/resampler.py:77-120) with dim_head = 64.
 * An executor handle: parameters through mve_unet_load_param under the module's state_dict() names (`latents`, `proj_in.*`,
 * `layers.N.0.{norm1,norm2}.*`, `layers.N.0.{to_q,to_kv,to_out}.weight`, `layers.N.1.0.*` (LayerNorm), `layers.N.1.{1,3}.weight`, `proj_out.*`,
 * `norm_out.*`).  Plan: proj_in; per layer norm1(x), norm2(latents), to_q on the latents, to_kv on the image rows and on the latent rows,
 * mve_attention with Lq = num_queries, first KV segment the n1 image keys, second segment the num_queries latent keys (the reference's
 * cat(x, latents) is never formed), to_out + residual, LayerNorm, bias-free Linear, GELU, bias-free Linear + residual; then proj_out and norm_out.
 * The ONE intended rounding difference: the reference scales q and k by dim_head^-1/4 each and rounds the softmax to 16 bit; here the logits are
 * scaled by 1/8 in fp32 and the probabilities are mve_attention's fp32 softmax.
 * dim, embedding_dim, output_dim multiples of 8; dim, output_dim <= 2048; the feed-forward width is dim * ff_mult.
 * d_x [B,n1,embedding_dim], d_out [B,num_queries,output_dim], both in the handle's dtype and 16-byte aligned. */
MVE_API int mve_ip_resampler_create(void** handle, int dtype, int dim, int depth, int heads, int num_queries, int embedding_dim, int output_dim,
                                    int ff_mult);
MVE_API int mve_ip_resampler_plan(void* handle, int B, int n1, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_ip_resampler_forward(void* handle, const void* d_x, int B, int n1, void* d_out, void* d_workspace, size_t workspace_bytes,
                                     float* op_ms, void* stream);
/* DPT-hybrid dense predictor (the reference's `normal_model`: DPTDepthModel over timm's vit_base_resnet50_384; the same architecture as transformers'
 * DPTForDepthEstimation with is_hybrid=True over a BitBackbone).  An executor handle; parameters through mve_unet_load_param under the ENGINE's slot
 * names, each a tensor of exactly the slot's size (mvedit_amd/normal_model.py maps checkpoint keys onto them and standardises the ResNetV2 weights
 * once, in float64, before the single rounding): `stem.w` [Cs][152]; `stem.{g,b}`; per bottleneck `sS.bM.{c1.w [mid][cin], c2.w (mve_conv3x3 K order),
 * c3.w [cout][mid], n1,n2,n3.{g,b}}` and for M = 0 `ds.w [cout][cin]`, `dn.{g,b}`; `proj.{w,b}`, `cls`, `pos`; per ViT block `lK.{n1,n2}.{g,b}`,
 * `lK.{qkv,o,fc1,fc2}.{w,b}`; `r3 / r4 .{wt,wc} [C][C]` (token / class halves of the readout Linear), `.b`, `.p.{w,b}`, `r4.z.{w,b}`; `rn1..4.w`;
 * `fK.{u1,u2}.{c1,c2}.{w,b}`, `fK.out.{w,b}` (no `f4.u1`); `h0.{w,b}`, `h2.{w,b}`, `h4.{w [8][32], b [8]}` (rows >= num_channels zero).
 * mve_unet_missing_params / mve_unet_op_info / mve_unet_destroy apply.
 * Plan (csrc/builder_dpt.h): mve_dpt_stem_rows + GEMM, GroupNorm + ReLU, mve_dpt_maxpool; bottlenecks (1 x 1 GEMM, GN + ReLU, 3 x 3 conv with the
 * stride and MVE_CONV_PAD_BR, GN + ReLU, 1 x 1 GEMM, GN; shortcut mve_dpt_gather_s2 + GEMM + GN; mve_dpt_add_relu); 1 x 1 projection,
 * mve_clip_vision_embed, pre-norm ViT blocks on mve_layernorm / GEMMs / mve_attention (head_dim 64) / mve_act(GELU) up to the second tapped block;
 * the "project" readout as one GEMM over the patch tokens with the class half as the epilogue's per-image row vector; the four `layerN_rn` convs;
 * four fusion blocks (ReLU, conv, ReLU, conv + residual; add; again; mve_dpt_upsample2x; 1 x 1 GEMM); the head; NHWC -> NCHW.
 * Refused at create: image_size not a multiple of 32, head_dim != 64, hidden > 2048, widths that are not multiples of 8 / of the group count,
 * num_channels > 8.  d_pixels [B,3,S,S] NCHW with S = image_size, d_out [B,num_channels,S,S] NCHW, both in the handle's dtype, 16-byte aligned.
 * d_taps: NULL, or 10 pointers (each may be NULL) that receive, in the handle's dtype: the stem output and the three stage outputs (NHWC), the
 * two tapped token tensors [B,T,C], the four fusion outputs in execution order refinenet4 .. refinenet1 (NHWC). */
MVE_API int mve_dpt_create(void** handle, int dtype, int image_size, int stem_width, const int* stage_widths, const int* stage_depths, int num_groups,
                           int hidden_size, int num_layers, int num_heads, int intermediate_size, const int* tap_layers, const int* neck_channels,
                           int features, int num_channels, float layer_norm_eps);
MVE_API int mve_dpt_plan(void* handle, int B, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_dpt_forward(void* handle, const void* d_pixels, int B, void* d_out, void* const* d_taps, void* d_workspace, size_t workspace_bytes,
                            float* op_ms, void* stream);
/* LoFTR feature matcher (the reference's `matcher`: loftr/loftr.py with `default_cfg` -- ResNetFPN_8_2 1 -> 128 -> [128, 196, 256], a 256-wide
 * 8-head linear-attention transformer over ['self', 'cross'] x 4, dual-softmax coarse matching, 5 x 5 fine windows with the coarse feature
 * concatenated, a 128-wide 8-head ['self', 'cross'] fine transformer, FineMatching).  An executor handle; parameters through mve_unet_load_param
 * under the ENGINE's slot names, each a tensor of exactly the slot's size (mvedit_amd/matcher.py maps the checkpoint's keys onto them, folds every
 * eval-mode BatchNorm into the convolution in front of it in float64 and pads the 196-wide stage to 200 channels with zeros): `stem.{w [128][56], b}`;
 * per BasicBlock `lS.bM.{c1,c2}.{w (mve_conv3x3 K order), b}` and for the strided ones `ds.{w [cout][cin], b}`; `l3oc.w`, `l2oc.w`, `l1oc.w` (1 x 1);
 * `l2oc2.0.{w,b}`, `l2oc2.3.w`, `l1oc2.0.{w,b}`, `l1oc2.3.w`; per encoder layer `cK.` / `fK.` `{q.w [C][C], kv.w [2C][C], merge.w [C][C],
 * mlp0.w [2C][2C], mlp2.w [C][2C], n1.{g,b}, n2.{g,b}}`; `dp.{w [128][256], b}`, `mf.{w [128][256], b}`.
 * The forward is two calls with one host read between them (the match count M shapes every fine output):
 *   mve_loftr_forward_coarse  d_images [2N,1,H,W] (image0 of the N pairs, then image1; the handle's dtype), H and W multiples of 8, at most 2048;
 *                             d_pos fp32 [H/8 * W/8][256] the position table.  d_io[0] feat_f [2N,H/2,W/2,128] and d_io[1] feat_c [2N,L,256] (handle
 *                             dtype; kept for the fine call), d_io[2] sim fp32 [N,L,ld] with ld = S rounded up to 8, d_io[3] conf fp32 [N,L,S],
 *                             d_io[4..6] b_ids / i_ids / j_ids int64 [N*L], d_io[7] mconf fp32 [N*L], d_io[8..9] mkpts0_c / mkpts1_c fp32 [N*L][2],
 *                             d_io[10] the match count int32 [1].  d_taps: NULL or 14 pointers (each may be NULL): stem, layer1, layer2 (200
 *                             channels, the last 4 zero), layer3, fpn_c (NHWC, 2N images), the tokens after the position add and after each of
 *                             the 8 layers ([2N,L,256]: feat0 of the N pairs, then feat1).
 *   mve_loftr_forward_fine    M >= 1 matches (host value; at most N*min(L,S), the capacity the plan is made for): reads d_io[0], [1], [4..6], [9];
 *                             writes d_io[11] expec_f fp32 [M][3] and d_io[12] mkpts1_f fp32 [M][2].  d_taps: NULL or 3 pointers: the unfolded
 *                             windows, the merged windows, the windows after the fine transformer ([2M,25,128]: window 0 of every match, then window 1).
 * thr / border are mve_dsmax_select's.  The linear attention leaves out the reference's V / S ... * S guard (fp32 accumulators). */
MVE_API int mve_loftr_create(void** handle, int dtype);
MVE_API int mve_loftr_plan(void* handle, int phase, int N, int H, int W, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_loftr_forward_coarse(void* handle, const void* d_images, const float* d_pos, int N, int H, int W, float thr, int border, void* const* d_io,
                                     void* const* d_taps, void* d_workspace, size_t workspace_bytes, float* op_ms, void* stream);
MVE_API int mve_loftr_forward_fine(void* handle, int N, int H, int W, int M, void* const* d_io, void* const* d_taps, void* d_workspace, size_t workspace_bytes,
                                   float* op_ms, void* stream);
MVE_API int mve_loftr_destroy(void* handle);
/* Segment Anything image encoder (segment_anything `ImageEncoderViT` = transformers `SamVisionEncoder`; the reference's
 * `predictor.model.image_encoder`, run once per request by `SamPredictor.set_image`).  The prompt encoder, the mask decoder and the mask
 * post-processing are NOT part of it (mve_sam_decoder_* below).  An executor handle: parameters through mve_unet_load_param under transformers' names
 * (`patch_embed.projection.*`, `pos_embed`, `layers.N.{layer_norm1,layer_norm2}.*`, `layers.N.attn.{qkv,proj}.*`,
 * `layers.N.attn.{rel_pos_h,rel_pos_w}`, `layers.N.mlp.{lin1,lin2}.*`, `neck.{conv1,conv2}.weight`, `neck.{layer_norm1,layer_norm2}.*`;
 * mvedit_amd/sam.py renames segment_anything's keys onto them).  A rel_pos table must have exactly 2n-1 rows (n = window_size, or the grid in
 * a global block): another length would need the reference's linear interpolation and is refused by the loader.
 * mve_unet_missing_params / mve_unet_op_info apply.
 * Plan (csrc/builder_sam.h), G = image_size / patch_size: mve_clip_patchify, patch GEMM with bias, mve_sam_pos_add (hidden state 0); per block
 * LayerNorm, [windowed: mve_sam_window_partition of the normalised map, zero-padded to a multiple of window_size], q|k|v GEMM,
 * mve_attention_relpos (scale = head_dim^-1/2; NS = B * windows with n = window_size, or NS = B with n = G for the blocks in
 * global_attn_indexes), [windowed: mve_sam_window_unpartition], proj GEMM + residual on the B G^2 kept rows, LayerNorm, lin1 GEMM,
 * mve_act(GELU), lin2 GEMM + residual; the neck: 1 x 1 GEMM C -> output_channels without bias, mve_layernorm over the pixels' channels
 * (LayerNorm2d, eps 1e-6), mve_conv3x3 without bias, mve_layernorm, NHWC -> NCHW.  GEMMs never split K: an item's result does not depend on B.
 * Refused at create: head_dim (hidden / heads) not 64 or 80, hidden > 2048, image_size % patch_size != 0, a grid above 64 x 64, window_size
 * larger than the grid, more than 64 blocks, mlp_dim or output_channels not a multiple of 8, output_channels > 2048, use_rel_pos = 0,
 * use_abs_pos = 0.
 * d_pixels [B,3,S,S] NCHW and d_out [B,output_channels,G,G] NCHW in the handle's dtype, 16-byte aligned.  d_hidden_states: NULL, or
 * num_layers + 1 pointers to [B,G,G,C] tensors in the handle's dtype -- entry 0 is patch_embed + pos_embed, entry k + 1 the output of block k. */
MVE_API int mve_sam_encoder_create(void** handle, int dtype, int image_size, int patch_size, int hidden_size, int num_layers, int num_heads, int mlp_dim,
                                   int window_size, const int* global_attn_indexes, int n_global, int output_channels, float layer_norm_eps,
                                   int use_rel_pos, int use_abs_pos);
MVE_API int mve_sam_encoder_plan(void* handle, int B, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_sam_encoder_forward(void* handle, const void* d_pixels, int B, void* d_out, void* const* d_hidden_states, void* d_workspace,
                                    size_t workspace_bytes, float* op_ms, void* stream);
MVE_API int mve_sam_encoder_destroy(void* handle);
/* Segment Anything prompt encoder + two-way mask decoder (transformers `SamPromptEncoder` + `SamMaskDecoder` = segment_anything's `PromptEncoder`
 * + `MaskDecoder`; what `SamPredictor.predict` runs per prompt).  fp32 throughout; `dtype` (f16 | bf16) is the dtype of the image
 * embedding it reads.  An executor handle: parameters through mve_unet_load_param under the names `SamModel.state_dict()` prints
 * (`shared_image_embedding.positional_embedding`, `prompt_encoder.{point_embed.N,not_a_point_embed,no_mask_embed}.weight`,
 * `mask_decoder.{iou_token,mask_tokens}.weight`, `mask_decoder.transformer.layers.N.{self_attn,cross_attn_token_to_image,
 * cross_attn_image_to_token}.{q,k,v,out}_proj.*`, `...layers.N.{layer_norm1..4,mlp.lin1,mlp.lin2}.*`, `mask_decoder.transformer.
 * {final_attn_token_to_image.*,layer_norm_final_attn.*}`, `mask_decoder.{upscale_conv1,upscale_conv2,upscale_layer_norm}.*`,
 * `mask_decoder.{output_hypernetworks_mlps.N,iou_prediction_head}.{proj_in,layers.0,proj_out}.*`; mvedit_amd/sam.py renames segment_anything's keys
 * onto them).  mve_sam_decoder_finalize runs mve_sam_dense_pe into the handle once the parameters are loaded; a forward before it is refused.
 * Plan (csrc/builder_sam_decoder.h, which restates the two-way transformer): one plan serves N = B * P items (B images, P prompts per image, one
 * prompt shape per call); mve_sam_prompt_tokens, mve_sam_src, then mve_gemm_f32 / mve_attention_f32 / mve_layernorm_f32 / mve_add_rows_f32,
 * mve_sam_upscale twice, mve_sam_token_mlps, mve_sam_mask_product.  No host read.
 * layer_norm_eps is that of layer_norm1..4, final_layer_norm_eps that of layer_norm_final_attn (transformers: 1e-6 / 1e-5; segment_anything: 1e-5
 * / 1e-5).  Refused at create: hidden_size / num_heads not 32 (and hidden_size / attention_downsample_rate / num_heads not 16),
 * attention_downsample_rate != 2, iou_head_depth != 3, iou_head_hidden_dim != hidden_size, hidden_size > 512 or not a multiple of 8,
 * num_mask_tokens outside [1, 8], more than 8 layers, a grid above 128.  Refused at plan / forward: more than 16 tokens, no prompt, N > 128.
 * d_embedding [B][hidden][G][G] NCHW in `dtype`; d_boxes NULL | fp32 [B*P][4] (x0, y0, x1, y1 in input-image pixels); d_points NULL | fp32
 * [B*P][n_points][2], d_labels int32 [B*P][n_points] in {-1, 0, 1}; d_low_res fp32 [B*P][num_mask_tokens][4G][4G], d_iou fp32
 * [B*P][num_mask_tokens] (ALL mask tokens: multimask_output selects [1:] or [:1] of them).  d_taps: NULL, or 2 * num_layers + 5 pointers, NULL
 * entries skipped: tokens [N][T][C]; per layer queries [N][T][C], keys [N][G^2][C]; queries after the final attention; the upscaled embedding
 * [N][16 G^2][C/8]; hyper_in [N][Mt][C/8]; the dense positional encoding [G^2][C]. */
MVE_API int mve_sam_decoder_create(void** handle, int dtype, int hidden_size, int num_layers, int num_heads, int mlp_dim, int num_mask_tokens, int iou_head_hidden_dim,
                                   int iou_head_depth, int attention_downsample_rate, int grid, int image_size, float layer_norm_eps, float final_layer_norm_eps);
MVE_API int mve_sam_decoder_finalize(void* handle, void* stream);
MVE_API int mve_sam_decoder_plan(void* handle, int B, int P, int n_points, int has_box, size_t* workspace_bytes, int* n_ops, double* flops);
MVE_API int mve_sam_decoder_forward(void* handle, const void* d_embedding, int B, int P, const float* d_boxes, const float* d_points, const int32_t* d_labels,
                                    int n_points, float* d_low_res, float* d_iou, void* const* d_taps, void* d_workspace, size_t workspace_bytes, float* op_ms,
                                    void* stream);
MVE_API int mve_sam_decoder_destroy(void* handle);
/* LPIPS(net='vgg') perceptual loss, forward and backward w.r.t. the prediction: the `patch_loss` of the reference's reconstruct step
 * (lib/models/losses/lpips_loss.py:8-42 -> lpips==0.1.4 `LPIPS.forward`; lib/models/autoencoders/base_nerf.py:337-344, 8 patches of
 * 128 x 128 per optimisation iteration).  An executor handle: parameters through mve_unet_load_param under lpips' own state-dict
 * names (`net.slice<k>.<idx>.weight|bias` = torchvision VGG16 features, `lin<k>.model.1.weight` (or `lins.<k>...`),
 * `scaling_layer.shift|scale`).  normalize_inputs: pred / target arrive in [0, 1] and are mapped to [-1, 1] first (LPIPSLoss default).
 *   forward : loss[n] = sum_l mean_hw sum_c w_lc (u_pred - u_target)^2, u = f / (|f|_c + 1e-10), f = relu{1_2,2_2,3_3,4_3,5_3};
 *             pred, target NCHW [B,3,H,W] in io_dtype, H and W multiples of 16; d_loss f32 [B].
 *   backward: d_grad_pred = d(sum_n grad_loss[n] loss[n]) / d pred, NCHW io_dtype; reads the activations the forward call left in
 *             d_workspace (same workspace, same B/H/W, nothing else run on it in between).  Every VGG conv's data gradient is the
 *             forward implicit-GEMM kernel on a transposed + flipped packing of the same weight. */
MVE_API int mve_lpips_create(void** handle, int dtype, int normalize_inputs);
MVE_API int mve_lpips_plan(void* handle, int B, int H, int W, int io_dtype, size_t* workspace_bytes, int* n_ops, int* n_forward_ops,
                           double* flops);
MVE_API int mve_lpips_forward(void* handle, const void* d_pred, const void* d_target, int io_dtype, int B, int H, int W, float* d_loss,
                              void* d_workspace, size_t workspace_bytes, void* stream);
MVE_API int mve_lpips_backward(void* handle, const float* d_grad_loss, int io_dtype, int B, int H, int W, void* d_grad_pred,
                               void* d_workspace, size_t workspace_bytes, void* stream);
/* LPIPS building blocks (csrc/lpips.hip), NHWC `dtype` activations:
 *   scale        : out[2B*H*W][8] = ((normalize ? 2x-1 : x) - shift_c) / scale_c of pred (first B images) and target, channels 3..7 zero
 *   input_grad   : d x[b][c][y][x] = g[(b,y,x)][c] / scale_c * (normalize ? 2 : 1), NCHW io_dtype
 *   maxpool2x2   : nn.MaxPool2d(2, 2) and its backward (gradient to the first arg-max of the window, as torch)
 *   relu_backward: grad = out > 0 ? grad : 0, in place
 *   lpips_layer  : loss[n] (+)= mean_hw sum_c w_c (u0 - u1)^2 over feat = [pred half | target half]; _backward: d / d feat(pred half) */
MVE_API int mve_lpips_scale(int dtype, int io_dtype, const void* d_pred, const void* d_target, int B, int H, int W, const float* d_shift3,
                            const float* d_scale3, int normalize, void* d_out, void* stream);
MVE_API int mve_lpips_input_grad(int dtype, int io_dtype, const void* d_g8, int B, int H, int W, const float* d_scale3, int normalize,
                                 void* d_out, void* stream);
MVE_API int mve_maxpool2x2(int dtype, const void* d_x, int B, int H, int W, int C, void* d_y, void* stream);
MVE_API int mve_maxpool2x2_backward(int dtype, const void* d_x, const void* d_grad_y, int B, int H, int W, int C, void* d_grad_x,
                                    void* stream);
MVE_API int mve_relu_backward(int dtype, void* d_grad, const void* d_out, size_t n, void* stream);
MVE_API size_t mve_lpips_layer_scratch_bytes(int B, int HW);
MVE_API int mve_lpips_layer(int dtype, const void* d_feat, const float* d_lin_w, int B, int HW, int C, int accumulate, float* d_loss,
                            void* d_scratch, void* stream);
MVE_API int mve_lpips_layer_backward(int dtype, const void* d_feat, const float* d_lin_w, const float* d_grad_loss, int B, int HW, int C,
                                     void* d_grad_feat, void* stream);
/* y = x >= 0 ? x : slope[c] * x over NHWC rows (nn.PReLU(num_parameters=C), image_space_ss.py:41-56); n = rows * C elements */
MVE_API int mve_prelu(int dtype, const void* d_x, const float* d_slope, int C, void* d_y, size_t n, void* stream);
/* out[b][c][y*r+i][x*r+j] = src[(b,y,x)][c*r*r + i*r + j] + base[b][c][y][x]: nn.PixelShuffle(r) of an NHWC fp32 tensor (row stride ld)
 * plus F.interpolate(base, scale_factor=r, mode='nearest') (image_space_ss.py:66-69); base and out NCHW in io_dtype. */
MVE_API int mve_pixel_shuffle_add(int io_dtype, const float* d_src, int ld, const void* d_base, int B, int C, int H, int W, int r,
                                  void* d_out, void* stream);

/* Tuning knob for engines created AFTER the call: 1 (default) folds every ResnetBlock2D conv_shortcut into conv2's K loop
 * (mve_conv3x3_shortcut), 0 keeps the separate 1x1 GEMMs; negative only queries.  Returns the previous setting. */
MVE_API int mve_unet_tune(int fuse_shortcut);
/* Opt-in hipGraph replay of mve_unet_forward (no reference counterpart; the reference launches every kernel eagerly): a forward whose
 * plan and every pointer argument (sample, timesteps, context, output, workspace, residuals, stream) equal those of an earlier call is
 * captured into a graph on its second sighting and replayed afterwards -- for launch-bound small-batch forwards (8 images per rank at
 * 8 GPUs).  Calls with op_ms (profiling) always run eagerly.  enable < 0 only queries; disabling frees the cached graphs.  Returns
 * the previous setting.  Off by default. */
MVE_API int mve_unet_graph(void* handle, int enable);

/* Attention-processor options of the reference, applied to every later plan/forward of this engine:
 *   ip_tokens > 0 : IPAttnProcessor2_0 (lib/models/architecture/ip_adapter/attention_processor.py:301-396) -- the last ip_tokens rows of
 *                   encoder_hidden_states are projected with `<block>.attn2.processor.to_k_ip/to_v_ip.weight` (loaded through
 *                   mve_unet_load_param under those names) and attended to in a second softmax, added with ip_scale.
 *   ref_mode      : ReferenceAttnProc (lib/models/architecture/diffusers.py:646-673) / ReferenceOnlyAttnProc
 *                   (lib/pipelines/zero123plus.py:43-77).  1 = mode 'w': every self-attention layer stores its keys/values;
 *                   2 = modes 'r' / 'm': every self-attention layer appends the stored tokens to its keys/values.  The first
 *                   ref_skip batch items neither store nor read (is_cfg_guidance).  ref_H x ref_W is the latent size of the
 *                   pass that wrote the store (mode 2 only).  d_ref_store is caller-owned device memory of at least
 *                   mve_unet_ref_store_bytes(B, ref_H, ref_W, ref_skip) bytes that must stay valid between the two passes. */
MVE_API int mve_unet_set_attention(void* handle, int ip_tokens, float ip_scale, int ref_mode, int ref_H, int ref_W, int ref_skip,
                                   void* d_ref_store, size_t ref_store_bytes);
/* Residual stream of the UNet / ControlNet executor (no reference counterpart: the reference's half modules round it after every block).
 * pair = 1: x + f(x) of ResnetBlock2D / BasicTransformerBlock / Transformer2DModel is carried as an unrounded (hi, lo) pair of 16-bit tensors -- the
 * residual adds, GroupNorm and LayerNorm read and write the pair, every MFMA operand reads `hi` -- which brings the end-to-end error of one SD-1.5
 * forward at 64 x 64 against fp32 arithmetic from 1.23e-3 to below north_star's 1e-3 (tests/rounding_budget_experiment.py predicts 7.0e-4) for
 * 4 more bytes per stream element and pass.  pair = 0 (default): the single 16-bit tensors of rounds 1-3.  Negative: query.  Returns the previous
 * mode; the mode is part of the plan key. */
MVE_API int mve_unet_set_residual_mode(void* handle, int pair);
/* CFG prefix of the UNet executor (no reference counterpart).  Under classifier-free guidance the batch is [uncond | text]: the reference builds it as
 * torch.cat([latents] * 2) with one timestep, so both halves enter the network identical and differ in encoder_hidden_states alone.  Every op in front
 * of the first cross-attention (SD-1.5: down_blocks.0.resnets.0 and the first transformer up to attn2.to_q, one of the five 4096-token self-attentions
 * among them; conv_in stays at full batch) then produces bit-identical rows for image b and image b + B / 2.  With the switch on (the default) a probe
 * kernel at the start of each forward compares the two halves of `sample` and of the time-embedding projection rows bit for bit and writes a device flag;
 * the blocks of those ops that belong to the second half return at once when it is 1, and one copy kernel hands the first half of the tensors that
 * outlive the prefix to the second.  The launches are the full-batch problem's either way (same tiles, same K slices), so the output is bit-identical
 * to the switch-off output for ANY input; nothing is decided on the host and a graph replay re-evaluates the flag.  Planned when B is even,
 * (B / 2) % num_cross_attn_imgs == 0 and reference attention is off; ControlNet handles are not covered.  on < 0: query.  Returns the previous value;
 * the switch is part of the plan key.  A handle of any kind but a UNet is MVE_ERR_ARG. */
MVE_API int mve_unet_tune_cfg_prefix(void* handle, int on);
/* Diagnostics (tests / tools): synchronises the stream of the last mve_unet_forward that ran a prologue and returns its flag -- 1: the halves were
 * identical and the prefix ran once, 0: they differed, -1: that plan had no prefix.  Errors are MVE_ERR_HIP, or MVE_ERR_STATE for a null handle (-1 is taken). */
MVE_API int mve_unet_cfg_prefix_state(void* handle);
/* SDXL added-condition embedding of a UNet or ControlNet handle (diffusers 0.27.2 UNet2DConditionModel / ControlNetModel with
 * addition_embed_type='text_time'; the reference passes `added_cond_kwargs` to both, lib/pipelines/adapter3d_mixin.py:99-125).  Mirrors
 *   time_embeds = self.add_time_proj(time_ids.flatten())                       # Timesteps(addition_time_embed_dim, True, 0), fp32
 *   add_embeds  = torch.concat([text_embeds, time_embeds.reshape(B, -1)], -1).to(emb.dtype)   # [B, projection_input_dim]
 *   emb         = emb + self.add_embedding(add_embeds)                         # TimestepEmbedding: linear_1, SiLU, linear_2
 * where `emb` is the output of time_embedding.linear_2.
 * mve_unet_set_addition_embed declares it: addition_type 1 = 'text_time' (0 = none), projection_input_dim = the in_features of
 * add_embedding.linear_1.  Call it after mve_unet_create / mve_controlnet_create and BEFORE the first mve_unet_load_param (MVE_ERR_STATE
 * afterwards): it adds add_embedding.linear_{1,2}.{weight,bias} to the parameter table and to the required names.  The addition type is
 * part of the plan key. */
MVE_API int mve_unet_set_addition_embed(void* handle, int addition_type, int addition_time_embed_dim, int projection_input_dim);
/* Binds the added conditions of the following forwards (mve_unet_forward phases 0 / 1, mve_controlnet_forward) of a 'text_time' handle:
 * caller-owned device memory d_text_embeds [B, text_dim] (text_dtype: f32 | f16 | bf16) and d_time_ids [B, n_ids] (f32), which are read by
 * every forward until the next call, so they must stay valid; text_dim + n_ids * addition_time_embed_dim must equal projection_input_dim
 * and B the forward's batch.  Both pointers NULL: unbind.  A 'text_time' handle run without a binding returns MVE_ERR_STATE (it never
 * embeds zeros); a binding on a handle without the embedding is MVE_ERR_STATE too.  Under mve_unet_graph the bound pointers and
 * widths are part of the graph key. */
MVE_API int mve_unet_bind_added_cond(void* handle, const void* d_text_embeds, int text_dtype, int text_dim, const float* d_time_ids, int n_ids,
                                     int B);
MVE_API size_t mve_unet_ref_store_bytes(void* handle, int B, int ref_H, int ref_W, int ref_skip);

/* (No reference counterpart: executor introspection, the source of bench.py's per-kernel roofline figures.)
 * op i of the cached plan: class, flops, label; returns 1 if the op belongs to unet_enc, 2 for unet_dec */
MVE_API int mve_unet_op_info(void* handle, int i, int* cls, double* flops, char* label, int label_len);

/* =========================================================================
 * 4. NeRF render path (float32 throughout, as in the reference).
 * ========================================================================= */

/* iNGPDecoder.point_decode (lib/models/decoders/ingp_decoder.py:106-120): tinycudann HashGrid (Smoothstep, 2 features
 * per level, log2_hashmap_size 19) -> MLP(2L -> hidden -> 4, ReLU) -> sigma = exp(h0 + blob(x)), rgb = sigmoid(h1..3)*(1+2s)-s.
 * level_* are HOST arrays [n_levels] (scale, resolution, row offset, row count per level; see oracle/nerf_oracle.py:grid_meta
 * for tiny-cuda-nn's formulas); d_table: [rows][2] f32; d_w1: [hidden][2L], d_w2: [4][hidden] (torch Linear layout).
 * d_rgbs may be NULL (point_density_decode). n_levels in {12, 14, 16}. */
MVE_API int mve_hashgrid_mlp_decode(const float* d_xyz, uint32_t M, const float* d_table, int n_levels,
                                    const float* level_scale, const uint32_t* level_res, const uint32_t* level_offset,
                                    const uint32_t* level_size, const float* d_w1, const float* d_b1, const float* d_w2,
                                    const float* d_b2, int hidden, float bound, float blob_density, float blob_radius,
                                    float sigmoid_saturation, float* d_sigmas, float* d_rgbs, void* stream);
/* Capacity form: the grid is sized by `capacity`; a row at or beyond *d_count (device int32) loads nothing and gets sigma = 0,
 * rgb = 0, so no consumer ever reads uninitialised memory.  Rows below the count equal mve_hashgrid_mlp_decode bit for bit. */
MVE_API int mve_hashgrid_mlp_decode_n(const float* d_xyz, uint32_t capacity, const int32_t* d_count, const float* d_table, int n_levels,
                                      const float* level_scale, const uint32_t* level_res, const uint32_t* level_offset,
                                      const uint32_t* level_size, const float* d_w1, const float* d_b1, const float* d_w2,
                                      const float* d_b2, int hidden, float bound, float blob_density, float blob_radius,
                                      float sigmoid_saturation, float* d_sigmas, float* d_rgbs, void* stream);

/* Decoder backward (the reconstruct step): gradients of  sum(g_sigma * sigma) + sum(g_rgb * rgb)  for the M
 * points of a training batch w.r.t. the hash table and the MLP of iNGPDecoder.point_decode (lib/models/decoders/ingp_decoder.py:106-120;
 * sigma uses the backward of the reference's _trunc_exp, lib/ops/activation.py:17-20).  The forward is recomputed, nothing has to be
 * saved.  d_grad_table [rows][2] is ACCUMULATED into (float atomics; zero it per optimiser step); the four MLP gradients are
 * overwritten (deterministic two-stage reduction).  d_grad_rgb may be NULL (density-only).  hidden must be 64. */
MVE_API size_t mve_hashgrid_mlp_backward_workspace_bytes(uint32_t M, int n_levels);
MVE_API int mve_hashgrid_mlp_backward(const float* d_xyz, uint32_t M, const float* d_table, int n_levels, const float* level_scale,
                                      const uint32_t* level_res, const uint32_t* level_offset, const uint32_t* level_size,
                                      const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2, int hidden, float bound,
                                      float blob_density, float blob_radius, float sigmoid_saturation, const float* d_grad_sigma,
                                      const float* d_grad_rgb, float* d_grad_table, float* d_grad_w1, float* d_grad_b1,
                                      float* d_grad_w2, float* d_grad_b2, void* d_workspace, size_t workspace_bytes, void* stream);
/* Capacity form: workspace >= mve_hashgrid_mlp_backward_workspace_bytes(capacity, n_levels); rows at or beyond *d_count contribute
 * nothing and are never read.  The fixed-order reduction runs over the live 256-row blocks only, in the exact call's order, so the four
 * MLP gradients equal mve_hashgrid_mlp_backward(M = count) bit for bit; the table gradient keeps its float atomics. */
MVE_API int mve_hashgrid_mlp_backward_n(const float* d_xyz, uint32_t capacity, const int32_t* d_count, const float* d_table, int n_levels,
                                        const float* level_scale, const uint32_t* level_res, const uint32_t* level_offset,
                                        const uint32_t* level_size, const float* d_w1, const float* d_b1, const float* d_w2,
                                        const float* d_b2, int hidden, float bound, float blob_density, float blob_radius,
                                        float sigmoid_saturation, const float* d_grad_sigma, const float* d_grad_rgb, float* d_grad_table,
                                        float* d_grad_w1, float* d_grad_b1, float* d_grad_w2, float* d_grad_b2, void* d_workspace,
                                        size_t workspace_bytes, void* stream);
/* torch.optim.Adam step (no weight decay, no amsgrad) in place on param / exp_avg / exp_avg_sq; step counts from 1. */
MVE_API int mve_adam_step(float* d_param, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, size_t n, float lr, float beta1,
                          float beta2, float eps, int step, void* stream);
/* The same step with its state on the device: *d_step (int32) counts the steps already taken, the launch applies step *d_step + 1
 * with the bias corrections computed in the kernel.  *d_skip != 0 (int32, e.g. the overflow flag of the capacity forward): the launch
 * changes nothing -- not the parameter, not the moments.  mve_adam_advance_n, once after the parameters of one optimiser step, adds one
 * to *d_step unless *d_skip != 0. */
MVE_API int mve_adam_step_n(float* d_param, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, size_t n, float lr, float beta1,
                            float beta2, float eps, const int32_t* d_step, const int32_t* d_skip, void* stream);
MVE_API int mve_adam_advance_n(int32_t* d_step, const int32_t* d_skip, void* stream);

/* VolumeRenderer.forward, eval branch (lib/models/decoders/base_volume_renderer.py:264-329) as ONE launch:
 * near/far from the aabb, occupancy-grid march (cascade count 1, no contraction, noise 0), hash-grid + MLP decode and
 * compositing per ray, with the reference's termination rules.  Outputs [N], [N], [N,3]; d_n_samples [N] optional. */
MVE_API int mve_nerf_render_rays(const float* d_rays_o, const float* d_rays_d, uint32_t N, const uint8_t* d_bitfield,
                                 uint32_t grid_size, const float* d_aabb, float bound, float min_near, float dt_gamma,
                                 uint32_t max_steps, float T_thresh, const float* d_table, int n_levels,
                                 const float* level_scale, const uint32_t* level_res, const uint32_t* level_offset,
                                 const uint32_t* level_size, const float* d_w1, const float* d_b1, const float* d_w2,
                                 const float* d_b2, int hidden, float blob_density, float blob_radius,
                                 float sigmoid_saturation, float* d_weights_sum, float* d_depth, float* d_image,
                                 int32_t* d_n_samples, void* stream);

/* get_ray_directions + get_rays(norm=True) (lib/core/utils/geometry_utils.py:18-55): intrinsics [V,4] (fx,fy,cx,cy),
 * poses [V,3,4] c2w -> rays_o, rays_d [V*h*w,3]; d_dir_norm [V*h*w] = |camera-space direction| (1/r -> 1/z factor), optional. */
MVE_API int mve_camera_rays(const float* d_intrinsics, const float* d_poses, int n_views, int h, int w, float* d_rays_o,
                            float* d_rays_d, float* d_dir_norm, void* stream);

/* depth_to_normal (geometry_utils.py:119-148, format 'opengl') fused with the tail of BaseNeRF.render
 * (lib/models/autoencoders/base_nerf.py:549-553): depth is 1/z; with d_alpha (element stride alpha_stride) the depth is
 * first divided by clamp(alpha,1e-6) and d_normal = normal_fg*alpha + normal_bg*(1-alpha).  normal_bg3: host [3] or NULL. */
MVE_API int mve_depth_to_normal(const float* d_depth, const float* d_alpha, int alpha_stride, const float* d_intrinsics,
                                int n_views, int h, int w, const float* normal_bg3, float* d_normal_fg, float* d_normal,
                                void* stream);

/* normalize_depth (geometry_utils.py:151-168): depths, alphas [V][hw] -> out [V][hw] */
MVE_API int mve_normalize_depth(const float* d_depths, const float* d_alphas, int n_views, int hw, float far_depth,
                                float alpha_clip, float eps, float* d_out, void* stream);

/* Stand-alone tinycudann HashGrid encoding (the `tcnn.Encoding` of lib/models/decoders/ingp_decoder.py:62-74 and
 * triplane_ingp_decoder.py:102-114; Python: mvedit_amd.tinycudann.Encoding).  d_x [N,3] f32 already in the unit cube (no bound applied);
 * d_table [n_rows][n_features] f32; level_* HOST arrays [n_levels] as mve_hashgrid_mlp_decode takes them, every level inside the
 * n_rows-row table and a hashed level 2^k rows; n_features in {1, 2, 4, 8}, 1 <= n_levels <= 16; interpolation MVE_INTERP_*.
 * Forward: d_out [N, n_levels * n_features] f32, row-major (level-major inside a row).  N = 0 is a no-op. */
#define MVE_INTERP_LINEAR 0
#define MVE_INTERP_SMOOTHSTEP 1
MVE_API int mve_hashgrid_encode(const float* d_x, uint32_t N, const float* d_table, uint32_t n_rows, int n_features, int n_levels,
                                const float* level_scale, const uint32_t* level_res, const uint32_t* level_offset,
                                const uint32_t* level_size, int interpolation, float* d_out, void* stream);
/* Backward of mve_hashgrid_encode for d_grad_enc = dL/denc [N, n_levels * n_features]: d_grad_table [n_rows][n_features] is
 * ACCUMULATED into (float atomics, as tiny-cuda-nn; same-cell neighbours are summed first); d_grad_x [N,3] = dL/dx is written when
 * not NULL (then d_table is read; Smoothstep's d w/dx = 6 t (1 - t) scale, Linear's = scale).  No second-order terms. */
MVE_API int mve_hashgrid_encode_backward(const float* d_x, uint32_t N, const float* d_table, uint32_t n_rows, int n_features,
                                         int n_levels, const float* level_scale, const uint32_t* level_res,
                                         const uint32_t* level_offset, const uint32_t* level_size, int interpolation,
                                         const float* d_grad_enc, float* d_grad_table, float* d_grad_x, void* stream);

/* =========================================================================
 * 5. Texture-space ops of the mesh path.
 * ========================================================================= */

/* edge_dilation (lib/ops/edge_dilation.py:5-47): img [n,c,h,w] f32, mask [n,1,h,w] f32 -> dilated img (and mask) after
 * `iters` rounds of nearest-valid-texel fill inside a (2*round(radius)+1)^2 window.  *_tmp: ping-pong scratch of the same
 * sizes (may be NULL when iters <= 1).  Inputs are not modified. */
MVE_API int mve_edge_dilation(const float* d_img, const float* d_mask, int n, int c, int h, int w, float radius, int iters,
                              float* d_img_out, float* d_mask_out, float* d_img_tmp, float* d_mask_tmp, void* stream);

/* =========================================================================
 * 6. Mesh rasterisation (output convention of nvdiffrast as used at
 *    lib/models/decoders/mesh_renderer/base_mesh_renderer.py:240-252; coverage rules specified in oracle/raster_oracle.c).
 * ========================================================================= */

/* dr.rasterize(glctx, pos, tri, (H, W)) as called at base_mesh_renderer.py:240-241, :521, :543:
 * pos: [B][V][4] clip-space f32, tri: [F][3] i32 -> rast [B][H][W][4] = (u, v, z/w, triangle_id+1), 0 where empty.
 * Row 0 is y_ndc = -1 (OpenGL orientation).  d_workspace: >= mve_rasterize_workspace_bytes(B,H,W,F). */
MVE_API size_t mve_rasterize_workspace_bytes(int B, int H, int W, int F);
MVE_API int mve_rasterize(const float* d_pos, int B, int V, const int32_t* d_tri, int F, int H, int W, float* d_rast,
                          void* d_workspace, size_t workspace_bytes, void* stream);
/* dr.interpolate(attr, rast, tri)[0] (base_mesh_renderer.py:246-252, :259, :265, :273, :545, :556, :573):
 * attr [Battr][Vattr][A] (Battr 1 broadcasts), tri [F][3] indexes attr; out [B][H][W][A], 0 where empty */
MVE_API int mve_interpolate(const float* d_attr, int Battr, int Vattr, int A, const float* d_rast, int B, int H, int W,
                            const int32_t* d_tri, int F, float* d_out, void* stream);

/* Multi-view texture back-projection, the device part of MeshRenderer.bake_multiview
 * (lib/models/decoders/mesh_renderer/base_mesh_renderer.py:507-603).  Bilinear filter with wrap addressing; the reference's
 * default 'linear-mipmap-linear' (nvdiffrast) is not reproduced -- see DESIGN.md.
 *   splat_visibility : sum of bilinear footprint weights of every foreground pixel (texc [n,h,w,2] uv, rast [n,h,w,4]) per
 *                      texel = d sum(texture(ones, texc)) / d ones (:547-552); d_vis_u64 [n][map][map] 2^-32 fixed point.
 *   view_weight      : clamp(-normal.dir, 0)^pow * alpha from the 1/z depth map, then the 5x5 min-pool (:554-566);
 *                      d_tmp and d_out are [n,h,w] f32.
 *   bake_accumulate  : per texel and view, fetch (rgb, view weight) at the texel's projected position (v_img [n,V,2] =
 *                      clip.xy/w*0.5+0.5 interpolated over the UV-space raster tex_rast [map,map,4] with faces d_f) and
 *                      add (rgb*weight, weight), weight = view_weight * visibility, into d_accum [map,map,4] (:568-582).
 *   bake_finalize    : albedo = sum / max(weight, 1e-8) -> [3][map][map] (ready for mve_edge_dilation). */
MVE_API int mve_splat_visibility(const float* d_texc, const float* d_rast, int n, int h, int w, int map_size, void* d_vis_u64,
                                 void* stream);
MVE_API int mve_view_weight(const float* d_depth, const float* d_alpha, const float* d_intrinsics, int n, int h, int w,
                            float cos_weight_pow, float* d_tmp, float* d_out, void* stream);
MVE_API int mve_bake_accumulate(const float* d_tex_rast, const int32_t* d_f, int F, const float* d_v_img, int V,
                                const float* d_images, const float* d_w_img, const void* d_vis_u64, int n, int h, int w,
                                int map_size, float* d_accum, void* stream);
MVE_API int mve_bake_finalize(const float* d_accum, int map_size, float* d_albedo_chw, void* stream);

/* Remaining pieces of MeshRenderer.forward (base_mesh_renderer.py:207-395):
 *   edge_opposites   : per triangle edge e = (tri[e], tri[(e+1)%3]) the vertex opposite to it in the one other triangle sharing the
 *                      edge, -1 for boundary / non-manifold edges (what dr.antialias derives from the topology) -> opp [F,3];
 *   antialias        : dr.antialias(color [B,h,w,C], rast, pos [B,V,4], tri) (:289-293) with the silhouette rules specified in
 *                      oracle/raster_oracle.c; d_out must not alias d_color;
 *   texture_bilinear : dr.texture(tex [Bt,th,tw,C] (Bt = 1 broadcasts), uv [n,h,w,2]) with the bilinear filter and wrap addressing;
 *                      pixels with rast[...,3] == 0 are written as 0 when d_rast is given (:258-263);
 *   box_downsample   : F.interpolate(mode='area', scale_factor=1/factor) on channel-last images (interpolate_hwc, :15-19, :380-383). */
MVE_API size_t mve_edge_opposites_workspace_bytes(int F);
MVE_API int mve_edge_opposites(const int32_t* d_tri, int F, int32_t* d_opp, void* d_workspace, size_t workspace_bytes, void* stream);
/* Capacity form (csrc/mesh_capacity_core.h): tri [f_cap,3], d_live = device int32 [2] (live vertices, live faces).  The edge table takes the
 * live faces only; rows of opp at or beyond the live face count are -1.  Workspace: mve_edge_opposites_workspace_bytes(f_cap). */
MVE_API int mve_edge_opposites_n(const int32_t* d_tri, int f_cap, const int32_t* d_live, int32_t* d_opp, void* d_workspace,
                                 size_t workspace_bytes, void* stream);
MVE_API int mve_antialias(const float* d_color, int B, int H, int W, int C, const float* d_rast, const float* d_pos, int V,
                          const int32_t* d_tri, int F, const int32_t* d_opp, float* d_out, void* stream);
MVE_API int mve_texture_bilinear(const float* d_tex, int Bt, int th, int tw, int C, const float* d_uv, const float* d_rast, int n, int h,
                                 int w, float* d_out, void* stream);
MVE_API int mve_box_downsample(const float* d_x, int B, int H, int W, int C, int factor, float* d_y, void* stream);

/* Marching tetrahedra, DMTet.__call__ (lib/models/decoders/mesh_renderer/base_mesh_renderer.py:140-188): pos [Nv,3] f32,
 * sdf [Nv] f32 (occupied where sdf > 0), tets [Nt,4] int32 -> verts [n_verts,3] f32 (one per sign-changing edge, in the
 * lexicographic order of the reference's torch.unique), faces [n_faces,3] int32 (one-triangle tets first, then two-triangle
 * tets, each in tet order).  Two calls because the sizes are data dependent: count writes (n_verts, n_faces) to d_counts
 * (device int32[2]); after reading them the caller allocates the outputs and calls write with the SAME untouched workspace. */
MVE_API size_t mve_dmtet_workspace_bytes(size_t n_verts, size_t n_tets);
MVE_API int mve_dmtet_count(const float* d_sdf, const int32_t* d_tets, size_t n_verts, size_t n_tets, int32_t* d_counts,
                            void* d_workspace, size_t workspace_bytes, void* stream);
MVE_API int mve_dmtet_write(const float* d_pos, const float* d_sdf, const int32_t* d_tets, size_t n_verts, size_t n_tets,
                            float* d_out_verts, int32_t* d_out_faces, int32_t* d_out_edges /* optional [n_out,2]: the grid edge
                            (a < b) behind every output vertex, what the backward needs */, void* d_workspace,
                            size_t workspace_bytes, void* stream);
/* Backward of the vertex interpolation (the part of DMTet.__call__ that carries gradients, base_mesh_renderer.py:167-176):
 * d_grad_pos [Nv,3] and d_grad_sdf [Nv] are ACCUMULATED into (float atomics; either may be NULL). */
MVE_API int mve_dmtet_backward(const float* d_pos, const float* d_sdf, const int32_t* d_edges, size_t n_out_verts,
                               const float* d_grad_verts, float* d_grad_pos, float* d_grad_sdf, void* stream);
/* Capacity (host-read-free) form, rules in csrc/mesh_capacity_core.h: count and write in ONE call into verts [v_cap,3], faces [f_cap,3]
 * and (optional) edges [v_cap,2], with the passes, the rounding and the vertex / face order of mve_dmtet_count + mve_dmtet_write.
 *   d_counts   int32 [2]  the true totals (n_verts, n_faces), also when they do not fit;
 *   d_overflow int32 [1]  1 when n_verts > v_cap or n_faces > f_cap, else 0;
 *   d_live     int32 [2]  (n_verts, n_faces) when nothing overflows, (0, 0) when anything does: the empty mesh, never a truncated one.
 * Rows at and beyond the live counts are written on every call: vertices 0.0, faces (0, 0, 0), edges (0, 0).
 * Workspace: mve_dmtet_workspace_bytes(n_verts, n_tets). */
MVE_API int mve_dmtet_extract_n(const float* d_pos, const float* d_sdf, const int32_t* d_tets, size_t n_verts, size_t n_tets, int v_cap,
                                int f_cap, float* d_out_verts, int32_t* d_out_faces, int32_t* d_out_edges, int32_t* d_counts,
                                int32_t* d_live, int32_t* d_overflow, void* d_workspace, size_t workspace_bytes, void* stream);
/* Backward over the live rows of edges [v_cap,2] / grad_verts [v_cap,3] (d_live as above; a padded (0, 0) edge is never read: its
 * s_a - s_b is 0).  d_grad_pos / d_grad_sdf are accumulated into, as in mve_dmtet_backward. */
MVE_API int mve_dmtet_backward_n(const float* d_pos, const float* d_sdf, const int32_t* d_edges, int v_cap, const int32_t* d_live,
                                 const float* d_grad_verts, float* d_grad_pos, float* d_grad_sdf, void* stream);

/* Backward of the render ops w.r.t. their colour-like input (mesh half): what nvdiffrast's autograd supplies
 * when the reference optimises textures / vertex colours through MeshRenderer.forward (lib/pipelines/mvedit_3d_pipeline.py:716-847,
 * lib/pipelines/mvedit_texture_pipeline.py optimisation loop).  The forward ops are linear in
 * that input, so these are their exact transposes; geometry (rast, pos) carries no gradient.
 *   interpolate_backward      : d_grad_attr [Battr,V,A] += barycentric weights * d_grad_out [B,h,w,A]   (accumulates; float atomics)
 *   texture_bilinear_backward : d_grad_tex [Bt,th,tw,C] += bilinear weights * d_grad_out [n,h,w,C]      (accumulates; float atomics)
 *   antialias_backward        : d_grad_color [B,h,w,C] = transpose of mve_antialias applied to d_grad_out (overwrites; deterministic) */
MVE_API int mve_interpolate_backward(const float* d_grad_out, int Battr, int Vattr, int A, const float* d_rast, int B, int H, int W,
                                     const int32_t* d_tri, int F, float* d_grad_attr, void* stream);
MVE_API int mve_texture_bilinear_backward(const float* d_grad_out, int Bt, int th, int tw, int C, const float* d_uv, const float* d_rast,
                                          int n, int h, int w, float* d_grad_tex, void* stream);
MVE_API int mve_antialias_backward(const float* d_grad_out, int B, int H, int W, int C, const float* d_rast, const float* d_pos, int V,
                                   const int32_t* d_tri, int F, const int32_t* d_opp, float* d_grad_color, void* stream);

/* Tri-plane radiance decoders: `TriPlaneDecoder.point_decode` (lib/models/decoders/triplane_decoder.py:135-199)
 * and `TriPlaneiNGPDecoder.point_decode` (lib/models/decoders/triplane_ingp_decoder.py:142-212) for one scene, forward (backward below):
 *   feature k = c * 3 + p of a point = bilinear F.grid_sample(padding_mode='border', align_corners=False) of channel c of plane p at the
 *   point's two coordinates for that plane (plane_cfg; flip_z negates z);  base_x = base_net(features) [+ ingp_base_net(hash-grid encoding
 *   of (xyz + bound) / (2 bound), tiny-cuda-nn HashGrid with Smoothstep interpolation)];  sigma = sigma_activation(density_net(act(base_x)));
 *   rgb = sigmoid(color_net(cat[act(base_x), SH_4(dir)])) * (1 + 2 s) - s.
 * Two topologies, selected by `topology`; both have base_net = one Linear(3C -> hidden), density_net = Linear(hidden -> 1), ingp_base_layers = 1:
 *   MVE_TRIPLANE_DEFAULT (0, the classes' constructor defaults; a descriptor filled as before this field existed):
 *       color_net = Linear(hidden + 16 -> hidden2), act, Linear(hidden2 -> 3) over cat[act(base_x), SH_4(dir)]; hidden, hidden2 in {64, 128}.
 *   MVE_TRIPLANE_DIRNET (1, what every config file of the reference asks for: dir_layers = [16, hidden], color_layers = [hidden, 3]):
 *       rgb = sigmoid(color_net(act(base_x + dir_net(SH_4(dir))))) * (1 + 2 s) - s with dir_net = Linear(16 -> hidden) in d_dir_wT / d_dir_b
 *       and color_net = ONE Linear(hidden -> 3) in d_col2_w / d_col2_b; hidden in {64, 128}; hidden2 and d_col1_* are ignored.
 * Weight matrices are passed TRANSPOSED ([in][out], fp32) so that a wave reads an input's fan-out as one contiguous scalar load.
 * code is channels-last [3][h][w][C].  activation: 0 relu, 1 silu, 2 softplus; sigma_activation: the same, 3 = trunc_exp (exp). */
typedef struct MveTriplaneDesc {
    const float *d_xyz, *d_dirs;                     /* [N,3]; d_dirs NULL: density only (point_density_decode) */
    const float *d_code;                             /* [3][h][w][C] */
    int32_t N, C, h, w;
    int32_t axes[6];                                 /* plane p reads (xyz[axes[2p]], xyz[axes[2p+1]]) */
    int32_t flip_z;
    const float *d_base_wT, *d_base_b;               /* [3C][hidden], [hidden] */
    int32_t hidden, hidden2;
    const float *d_ingp_wT, *d_ingp_b;               /* [2 n_levels][hidden], [hidden]; NULL for TriPlaneDecoder */
    const float *d_table;                            /* hash table [rows][2] */
    int32_t n_levels;
    float bound;
    const float *level_scale;                        /* HOST arrays [n_levels] (as mve_hashgrid_mlp_decode takes them) */
    const uint32_t *level_res, *level_offset, *level_size;
    const float *d_dens_w, *d_dens_b;                /* [hidden], [1] */
    const float *d_col1_wT, *d_col1_b;               /* [hidden + 16][hidden2], [hidden2] */
    const float *d_col2_w, *d_col2_b;                /* [3][hidden2], [3] */
    int32_t activation, sigma_activation;
    float sigmoid_saturation;
    float *d_sigmas, *d_rgbs;                        /* [N], [N,3] (d_rgbs unused when d_dirs is NULL) */
    int32_t topology;                                /* MVE_TRIPLANE_DEFAULT / MVE_TRIPLANE_DIRNET */
    const float *d_dir_wT, *d_dir_b;                 /* dir-net topology: [16][hidden], [hidden]; must be NULL for the default topology */
} MveTriplaneDesc;
#define MVE_TRIPLANE_DEFAULT 0
#define MVE_TRIPLANE_DIRNET 1
MVE_API int mve_triplane_decode(const MveTriplaneDesc* desc, void* stream);
/* Backward of mve_triplane_decode: gradients of sum(d_grad_sigmas * sigma) + sum(d_grad_rgbs * rgb) (d_grad_rgbs NULL: density only) -- what
 * autograd supplies when nerf_optim optimises a TriPlaneiNGPDecoder scene (lib/pipelines/mvedit_3d_pipeline.py:507-633 through
 * triplane_ingp_decoder.py:142-212; trunc_exp backward as lib/ops/activation.py:17-20).  Weight gradients come in the torch layout of the
 * reference modules ([out][in], OVERWRITTEN, reduced in a fixed order); d_code [3][h][w][C] and d_table [rows][2] are ACCUMULATED into
 * (float atomics, like F.grid_sample's / tiny-cuda-nn's backward; either may be NULL).  The forward is recomputed: desc's outputs are not
 * read or written. */
typedef struct MveTriplaneGrads {
    float *d_code, *d_table;
    float *d_base_w, *d_base_b;                      /* [hidden][3C], [hidden] */
    float *d_ingp_w, *d_ingp_b;                      /* [hidden][2 n_levels], [hidden] (NULL without a hash branch) */
    float *d_dens_w, *d_dens_b;                      /* [1][hidden], [1] */
    float *d_col1_w, *d_col1_b;                      /* [hidden2][hidden + 16], [hidden2] */
    float *d_col2_w, *d_col2_b;                      /* [3][hidden2], [3]; dir-net topology: color_net's one Linear, [3][hidden], [3] */
    float *d_dir_w, *d_dir_b;                        /* dir-net topology only: [hidden][16], [hidden] (d_col1_* are not read then) */
} MveTriplaneGrads;
/* With d_grad_rgbs NULL the colour-net (and dir_net) gradients are left untouched.  The workspace size depends on the topology: the dir-net
 * one has its own query (no hidden2). */
MVE_API size_t mve_triplane_backward_workspace_bytes(int N, int C, int hidden, int hidden2, int n_levels);
MVE_API size_t mve_triplane_dirnet_backward_workspace_bytes(int N, int C, int hidden, int n_levels);
MVE_API int mve_triplane_backward(const MveTriplaneDesc* desc, const float* d_grad_sigmas, const float* d_grad_rgbs, const MveTriplaneGrads* grads,
                                  void* d_workspace, size_t workspace_bytes, void* stream);
/* VolumeRenderer.forward, eval branch (lib/models/decoders/base_volume_renderer.py:264-329) over a tri-plane scene as ONE launch: near/far from
 * the aabb, occupancy-grid march (cascade count 1, no contraction, noise 0), the decode of mve_triplane_decode per occupied sample (both
 * topologies, hidden / hidden2 in {64, 128}, n_levels in {0, 12, 14, 16}) and compositing per ray with mve_nerf_render_rays' arithmetic and
 * termination rules.  What depends on the ray's direction alone (SH_4(d) and its product with dir_net / the SH rows of color_net.0) is computed
 * once per ray, so the sums run in another order than mve_triplane_decode's: close to, not bit-identical with, a render built on it.
 * The descriptor is read as mve_triplane_decode reads it, except that d_xyz, d_dirs, N, d_sigmas and d_rgbs are ignored, the colour net is
 * always needed and `bound` (the half-extent of the marched cube) must be set whether or not there is a hash grid.
 * Outputs [N], [N] (sum of w / t), [N,3]; d_n_samples [N] optional.  Deterministic; a ray's result does not depend on the other rays. */
MVE_API int mve_triplane_render_rays(const MveTriplaneDesc* desc, const float* d_rays_o, const float* d_rays_d, uint32_t N,
                                     const uint8_t* d_bitfield, uint32_t grid_size, const float* d_aabb, float min_near, float dt_gamma,
                                     uint32_t max_steps, float T_thresh, float* d_weights_sum, float* d_depth, float* d_image,
                                     int32_t* d_n_samples, void* stream);

/* Mip-mapped texture path: what the reference gets from nvdiffrast with MeshRenderer(texture_filter='linear-mipmap-linear') -- its default
 * (lib/models/decoders/mesh_renderer/base_mesh_renderer.py:196) -- in forward (:241, :260-264, :357-361), get_cam_weights_uv (:442, :466-475,
 * :496-500) and bake_multiview (:521, :543-552, :573-577).  nvdiffrast is not vendored: algorithm restated in oracle/texture_mip_oracle.py.
 *   rasterize_db        dr.rasterize(...)[1]: d_rast_db [B,H,W,4] = (du/dX, du/dY, dv/dX, dv/dY) of the barycentrics, 0 on empty pixels
 *   interpolate_da      dr.interpolate(attr, rast, tri, rast_db=..., diff_attrs='all')[1]: d_out [B,npix,2C] = (dA0/dX, dA0/dY, dA1/dX, ...)
 *   mip_levels          number of levels above level 0 of the full stack (down to 1 x 1); mip_texels = texels of levels 1..max_level
 *   mip_build           d_mips [Bt][mip_texels*C]: level l+1 = 2x2 box filter of level l (extents must be even at every level, or 1)
 *   texture_mip         dr.texture(tex [Bt,H,W,C], uv [n,h,w,2], uv_da [n,h,w,4], filter_mode='linear-mipmap-linear'), wrap addressing;
 *                       Bt = 1 broadcasts; pixels with rast[..,3] == 0 give 0 when d_rast is given (albedo[~fg] = 0, :264); C <= 8
 *   texture_mip_backward  gradient w.r.t. the texture: overwrites d_g_tex0 [Bt,H,W,C]; d_g_mips is scratch of the mip stack's size
 *   visibility_mip      `visibility_grad` (:470-475, :547-552): d sum(dr.texture(ones [n,map,map,1], texc, uv_da)) / d ones per view, accumulated
 *                       in 2^-32 fixed point (order independent) -> d_vis [n,map,map] fp32
 *   bake_accumulate_mip per texel and view: mip-mapped fetch of (rgb, view weight) from d_img0 [n,h,w,4] (+ its mip stack) at the texel's
 *                       projection, times d_vis; d_accum [map,map,4] += (rgb * weight, weight)   (:573-582) */
MVE_API int mve_rasterize_db(const float* d_pos, int B, int V, const int32_t* d_tri, int F, const float* d_rast, int H, int W,
                             float* d_rast_db, void* stream);
MVE_API int mve_interpolate_da(const float* d_attr, int attr_batch, int V, int C, const float* d_rast, const float* d_rast_db, int B, int npix,
                               const int32_t* d_tri, int F, float* d_out, void* stream);
MVE_API int mve_mip_levels(int H, int W);
MVE_API size_t mve_mip_texels(int H, int W, int max_level);
MVE_API int mve_mip_build(const float* d_tex0, int Bt, int H, int W, int C, int max_level, float* d_mips, void* stream);
MVE_API int mve_texture_mip(const float* d_tex0, const float* d_mips, int Bt, int H, int W, int C, int max_level, const float* d_uv,
                            const float* d_uv_da, const float* d_rast, int n, int h, int w, float* d_out, void* stream);
MVE_API int mve_texture_mip_backward(const float* d_g_out, int Bt, int H, int W, int C, int max_level, const float* d_uv,
                                     const float* d_uv_da, const float* d_rast, int n, int h, int w, float* d_g_tex0, float* d_g_mips,
                                     void* stream);
MVE_API size_t mve_visibility_mip_workspace_bytes(int n, int map_size, int max_level);
MVE_API int mve_visibility_mip(const float* d_texc, const float* d_texc_da, const float* d_rast, int n, int h, int w, int map_size,
                               int max_level, void* d_workspace, size_t workspace_bytes, float* d_vis, void* stream);
MVE_API int mve_bake_accumulate_mip(const float* d_tex_rast, const float* d_tex_rast_db, const int32_t* d_f, int F, const float* d_v_img,
                                    int V, const float* d_img0, const float* d_img_mips, int h, int w, int max_level, const float* d_vis,
                                    int n, int map_size, float* d_accum, void* stream);

/* Geometry gradients of dr.rasterize / dr.interpolate (nvdiffrast backward as the reference's mesh optimisation uses it through
 * MeshRenderer.forward, base_mesh_renderer.py:240-252):
 *   interpolate_backward_rast: grad_rast[pixel] = (sum_a g_a (a0 - a2), sum_a g_a (a1 - a2), 0, 0)   -- d out / d (u, v)
 *   rasterize_backward       : grad_pos[b][vertex] += d (u, v, z/w)[pixel] / d clip-space vertex, every pixel's triangle held fixed
 *                              (continuous barycentrics; float atomics; the caller zero-fills d_grad_pos [B][V][4]). */
MVE_API int mve_interpolate_backward_rast(const float* d_attr, int Battr, int Vattr, int A, const float* d_rast, int B, int H, int W,
                                          const int32_t* d_tri, int F, const float* d_grad_out, float* d_grad_rast, void* stream);
MVE_API int mve_rasterize_backward(const float* d_pos, int B, int V, const int32_t* d_tri, int F, int H, int W, const float* d_rast,
                                   const float* d_grad_rast, float* d_grad_pos, void* stream);
/* dr.antialias backward w.r.t. the clip-space vertices (the silhouette gradient): with the pair decisions of the forward held fixed,
 * out[dst] = c[dst] + |tt - 1/2| (c[src] - c[dst]) and tt is a smooth function of the crossed edge's two vertices.  grad_pos [B][V][4]
 * is accumulated with float atomics (caller zero-fills or chains it after mve_rasterize_backward). */
MVE_API int mve_antialias_backward_pos(const float* d_color, const float* d_grad_out, int B, int H, int W, int C, const float* d_rast,
                                       const float* d_pos, int V, const int32_t* d_tri, int F, const int32_t* d_opp, float* d_grad_pos,
                                       void* stream);

/* Geometry gradient of the texture path (csrc/texture_grad.hip; what mvedit_amd.nvdiffrast.torch adds to the ops above): the derivative
 * of the forward formulas of csrc/texmip_core.h with the tap indices, the level pair and every pixel's triangle held fixed.
 *   texture_grad_uv         d <g_out, dr.texture(tex, uv, uv_da)> / d uv -> d_g_uv [n,h,w,2] and / d uv_da -> d_g_uv_da [n,h,w,4] (either may be
 *                           NULL).  d_uv_da NULL: filter_mode='linear' (d_mips / max_level unused, d_g_uv_da must be NULL); otherwise
 *                           'linear-mipmap-linear' with the level stack of mve_mip_build.  d_g_uv_da is 0 where the level is clamped
 *                           (magnification, top level); at an exactly isotropic footprint the square root's term is taken as 0.  No rast
 *                           argument: every pixel is differentiated at its uv.  Bt = 1 broadcasts; any C.  Gathers only, no atomics.
 *   interpolate_da_backward from d_g_da [B,npix,2C]: d_g_rast_db [B,npix,4] is overwritten (0 on empty pixels); d_g_attr [attr_batch,V,C] is
 *                           ADDED to with float atomics (the buffer mve_interpolate_backward adds into).  Either may be NULL.
 *   rasterize_db_backward   from d_g_db [B,H,W,4]: the direct dependence of rast_db on the triangle's clip (x, y, w) is ADDED to d_g_pos
 *                           [B,V,4] with float atomics; its dependence on the stored (b0, b1) overwrites d_g_rast [B,H,W,4] (channels 2, 3
 *                           zero), to be added to the gradient of rast and passed to mve_rasterize_backward.  Either may be NULL. */
MVE_API int mve_texture_grad_uv(const float* d_tex0, const float* d_mips, int Bt, int H, int W, int C, int max_level, const float* d_uv,
                                const float* d_uv_da, const float* d_g_out, int n, int h, int w, float* d_g_uv, float* d_g_uv_da,
                                void* stream);
MVE_API int mve_interpolate_da_backward(const float* d_attr, int attr_batch, int V, int C, const float* d_rast, const float* d_rast_db, int B,
                                        int npix, const int32_t* d_tri, int F, const float* d_g_da, float* d_g_rast_db, float* d_g_attr,
                                        void* stream);
MVE_API int mve_rasterize_db_backward(const float* d_pos, int B, int V, const int32_t* d_tri, int F, const float* d_rast, int H, int W,
                                      const float* d_g_db, float* d_g_pos, float* d_g_rast, void* stream);

/* TRACER-B7 foreground segmentor (lib/models/segmentors/tracer_b7.py:16-73, called once per denoise step from
 * lib/pipelines/adapter3d_mixin.py:14-19; EfficientNet-B7 encoder lib/models/architecture/tracerb7/efficientnet.py + TRACER decoder
 * tracer.py / att_modules.py / conv_modules.py): the operators the GEMM / 3x3-conv entry points do not cover.  Activations are NHWC
 * 16-bit ([B, H, W, C] contiguous: a 1x1 convolution is mve_gemm on [B*H*W, C]); single-channel decoder maps are fp32; BatchNorm
 * arrives folded into weights + bias (mvedit_amd/segmentor.py folds it when the state dict is loaded).  act: 0 none, 1 swish,
 * 2 SELU, 3 ReLU, 4 sigmoid.
 *   seg_conv2d      : nn.Conv2d with groups = C (depthwise = 1: weights [kh][kw][C] f32; the _depthwise_conv of MBConvBlock,
 *                     efficientnet.py:66-75, with the STATIC TensorFlow-"SAME" padding of effi_utils.py:270-315 passed as explicit
 *                     top / left padding, and DWConv / DWSConv of conv_modules.py:42-88) or groups = 1 (weights [Cout][kh][kw][Cin] f32:
 *                     BasicConv2d with 1xk / kx1 / dilated kernels, conv_modules.py:11-39, att_modules.py:16-41).  out = act(conv + bias)
 *                     [* mul] [+ add]; x / out / mul / add rows are ldx / ldo / ld2 channels wide (channel slices of wider tensors).
 *   seg_act         : in-place activation of a GEMM / conv3x3 output (the swish / SELU behind a BatchNorm).
 *   seg_mconv       : small dense convolutions (stride 1, output size = input size) on the matrix cores with everything around them fused:
 *                     out[m][n] = act(sum_{tap, c} (x[pixel(m) + tap][c] * gate[b][c]) W[n][tap][c] + bias[n]) (+ residual[m][n]); W [N][ldw]
 *                     dtype with rows [kh][kw][Cin]; gate [B][Cin] f32 or NULL (1 x 1 only: the squeeze-and-excite scaling of
 *                     MBConvBlock.forward, efficientnet.py:124-131, applied to the operand in registers).  The expand conv + swish (:110-113),
 *                     the project conv + skip (:131-141), and the RFB block's 1 x 1, 1 x k, k x 1 and dilated 3 x 3 BasicConv2d layers
 *                     (conv_modules.py / att_modules.py:23-72; Cin % 32 == 0 when the kernel has taps).  Alignment: d_x, d_w 16 bytes;
 *                     d_out / d_residual 8 bytes, and 16 when ldo / ldr are multiples of 8 (rows are then stored 32 bytes per lane).
 *   seg_channel_mean: F.adaptive_avg_pool2d(x, 1) / GlobalAvgPool -> f32 [B][C].
 *   seg_se_gate     : sigmoid(_se_expand(swish(_se_reduce(pooled)))) (efficientnet.py:124-129), w1 [S][C], w2 [C][S] f32; pooled[b][c] = scale *
 *                     sum_k sums[b][k][c] (nslab = 1, scale = 1: a pooled vector as it is); d_hidden: [B][S + C] f32 workspace.
 *   seg_dwconv_pool : the MBConv block's depthwise convolution + swish (efficientnet.py:115-121) that also leaves the per-channel sums of its
 *                     (rounded) output per pixel slab, d_sums [B][seg_dwconv_slabs(B, Ho, Wo, C, k, stride)][C] f32 -- the squeeze without a second pass.
 *   seg_scale       : x = src * A[b][c] (+ S[b][c]) -- the SE gating; UnionAttentionModule's x * att + x, BatchNorm and confidence mask.
 *   seg_resize      : bilinear F.interpolate / torchvision Resize(antialias=False) (align_corners flag); in_mode 0: NHWC dtype, 1: NHWC
 *                     f32, 2: NCHW f32; optional (x - mean[c]) / std[c] (transforms.Normalize, tracer_b7.py:39-44).
 *   seg_uam_channel : UnionAttentionModule.channel_tracer + masking (att_modules.py:135-168) on the pooled vector; C <= 256.  Outputs the
 *                     sigmoid gate att and the per-(image, channel) affine A, S with BatchNorm(x * att + x) * mask = x * A + S (:163-174).
 *   seg_mul         : elementwise x * y (* z) (Aggregation.forward's gating products, att_modules.py:226-233).
 *   seg_uam_spatial : the spatial SDPA of UnionAttentionModule.forward (:176-187) over qkv [B][H*W][3] f32.
 *   seg_object_mix  : ObjectAttention's masked encoder map (att_modules.py:277-282).
 *   seg_fuse        : sigmoid((up4(d2) + up8(d1) + up8(d0)) / 3) (tracer.py:86-97).
 *   seg_post        : -max_pool2d(-m, 2 e + 1), resize to [Ho][Wo], failure rule (tracer_b7.py:66-72); out [B][Ho][Wo] dtype or f32. */
MVE_API int mve_seg_conv2d(int dtype, const void* d_x, int B, int H, int W, int Cin, int ldx, const float* d_w, const float* d_bias, void* d_out,
                           int Ho, int Wo, int Cout, int ldo, int kh, int kw, int stride, int pad_t, int pad_l, int dil, int depthwise, int act,
                           const void* d_mul, const void* d_add, int ld2, int out_f32, void* stream);
MVE_API int mve_seg_mconv(int dtype, const void* d_x, int B, int H, int W, int Cin, int ldx, const void* d_w, int ldw, int kh, int kw, int dil,
                          int pad_t, int pad_l, const float* d_bias, const float* d_gate, const void* d_residual, int ldr, void* d_out, int N,
                          int ldo, int act, void* stream);
MVE_API int mve_seg_act(int dtype, void* d_x, size_t n, int act, void* stream);
MVE_API int mve_seg_channel_mean(int dtype, const void* d_x, int B, int HW, int C, float* d_out, void* stream);
MVE_API int mve_seg_se_gate(const float* d_sums, int nslab, float scale, int B, int C, int S, const float* d_w1, const float* d_b1, const float* d_w2,
                            const float* d_b2, float* d_hidden, float* d_gate, void* stream);
MVE_API int mve_seg_dwconv_slabs(int B, int Ho, int Wo, int C, int k, int stride);
MVE_API int mve_seg_dwconv_pool(int dtype, const void* d_x, int B, int H, int W, int C, int ldx, const float* d_w, const float* d_bias, void* d_out, int Ho,
                                int Wo, int ldo, int kh, int kw, int stride, int pad_t, int pad_l, int act, float* d_sums, void* stream);
MVE_API int mve_seg_scale(int dtype, void* d_x, const void* d_src, int B, int HW, int C, const float* d_A, const float* d_S, void* stream);
MVE_API int mve_seg_resize(int dtype, const void* d_x, int B, int H, int W, int C, void* d_out, int Ho, int Wo, int align_corners, int in_mode,
                           int out_f32, const float* d_mean, const float* d_std, void* stream);
MVE_API int mve_seg_uam_channel(const float* d_pooled, int B, int C, const float* d_ns, const float* d_nb, const float* d_wq, const float* d_wk,
                                const float* d_wv, const float* d_wfc, float ratio, const float* d_bn_scale, const float* d_bn_shift, float* d_att,
                                float* d_A, float* d_S, void* stream);
MVE_API int mve_seg_mul(int dtype, const void* d_x, const void* d_y, const void* d_z, void* d_out, size_t n, void* stream);
MVE_API int mve_seg_uam_spatial(const float* d_qkv, int B, int H, int W, float* d_out, void* stream);
MVE_API int mve_seg_object_mix(int dtype, const float* d_map, const void* d_enc, void* d_out, int B, int HW, int C, void* stream);
MVE_API int mve_seg_fuse(const float* d_d0, const float* d_d1, const float* d_d2, int B, int Hs, int Ws, float* d_out, void* stream);
MVE_API size_t mve_seg_post_workspace_bytes(int B, int Hs, int Ws, int Ho, int Wo);
MVE_API int mve_seg_post(int dtype, const float* d_m, int B, int Hs, int Ws, int erosion, void* d_out, int Ho, int Wo, int out_f32,
                         void* d_workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVEDIT_AMD_H */
