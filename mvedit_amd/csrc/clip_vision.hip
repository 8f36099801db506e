// CLIP vision tower primitives (include/mvedit_amd.h section 2d): the operand rows of the patch convolution and the class + position
// embedding sum.  They replace the arithmetic of transformers' CLIPVisionEmbeddings (models/clip/modeling_clip.py) that the reference reaches
// through `IPAdapter.image_encoder` (lib/models/architecture/ip_adapter/ip_adapter.py:51-53, :130, :138), `Zero123PlusPipeline.vision_encoder`
// (lib/pipelines/zero123plus.py:372) and `Zero123Pipeline.image_encoder` (lib/pipelines/zero123.py:260).  Everything else of the tower is the
// executor's GEMMs, mve_layernorm, mve_act and mve_attention (csrc/builder_clip_vision.h).  Not the hot loop: written to be read, not tuned.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// patchify: rows[b*G*G + gy*G + gx][(c, ky, kx)] = pixels[b][c][gy*P + ky][gx*P + kx], columns [3*P*P, ld) zero; one thread per 8 columns.
// P % 8 == 0: the 8 columns are 8 consecutive pixels of one image row, 16-byte aligned (W = G*P) -- one vector load.  Otherwise 8 element loads.
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_clip_patchify(const typename Tag::T* __restrict__ px, typename Tag::T* __restrict__ rows, int H, int P, int G, int ld8,
                                                       long long total) {
    typedef typename Tag::T T;
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / ld8;
    const int k0 = (int)(i - row * ld8) * 8, PP = P * P, K = 3 * PP;
    const int b = (int)(row / ((long long)G * G)), g = (int)(row - (long long)b * G * G), gy = g / G, gx = g - gy * G;
    const T* img = px + (size_t)b * 3 * H * H;
    V8 o;
    if ((P & 7) == 0) {           // K is a multiple of 8 too: no tail
        const int c = k0 / PP, r = k0 - c * PP, ky = r / P, kx = r - ky * P;
        o = *reinterpret_cast<const V8*>(img + ((size_t)c * H + gy * P + ky) * H + gx * P + kx);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + e;
            T v = (T)0.f;
            if (k < K) {
                const int c = k / PP, r = k - c * PP, ky = r / P, kx = r - ky * P;
                v = img[((size_t)c * H + gy * P + ky) * H + gx * P + kx];
            }
            o[e] = v;
        }
    }
    reinterpret_cast<V8*>(rows)[i] = o;
}

template <class Tag>
int launch_clip_patchify(const void* px, void* rows, int B, int H, int P, int ld, hipStream_t s) {
    typedef typename Tag::T T;
    const int G = H / P;
    const long long total = (long long)B * G * G * (ld / 8);
    k_clip_patchify<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>((const T*)px, (T*)rows, H, P, G, ld / 8, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// embedding: out[b, 0, :] = cls + pos[0]; out[b, 1 + p, :] = patch[b, p, :] + pos[1 + p]; one thread per 8 channels
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_clip_vision_embed(const typename Tag::T* __restrict__ patch, const typename Tag::T* __restrict__ cls,
                                                           const typename Tag::T* __restrict__ pos, typename Tag::T* __restrict__ out, int G2, int C8, long long total) {
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / C8;
    const int c8 = (int)(i - row * C8), T1 = G2 + 1;
    const long long b = row / T1;
    const int t = (int)(row - b * T1);
    const V8 a = t == 0 ? reinterpret_cast<const V8*>(cls)[c8] : reinterpret_cast<const V8*>(patch)[((size_t)b * G2 + (t - 1)) * C8 + c8];
    const V8 e = reinterpret_cast<const V8*>(pos)[(size_t)t * C8 + c8];
    V8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = Tag::from_f32(Tag::to_f32(a[k]) + Tag::to_f32(e[k]));
    reinterpret_cast<V8*>(out)[i] = o;
}

template <class Tag>
int launch_clip_vision_embed(const void* patch, const void* cls, const void* pos, void* out, int B, int G2, int C, hipStream_t s) {
    typedef typename Tag::T T;
    const long long total = (long long)B * (G2 + 1) * (C / 8);
    k_clip_vision_embed<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>((const T*)patch, (const T*)cls, (const T*)pos, (T*)out, G2, C / 8, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mve_clip_patchify(int dtype, const void* pixels, int B, int H, int W, int P, void* rows, int ld, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "clip_patchify: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(pixels && rows, MVE_ERR_ARG, "clip_patchify: null pointer (d_pixels / d_rows)");
    MVE_CHECK(B >= 1 && H >= 1 && P >= 1 && P <= H, MVE_ERR_ARG, "clip_patchify: bad B %d / H %d / P %d", B, H, P);
    MVE_CHECK(W == H, MVE_ERR_ARG, "clip_patchify: W %d must equal H %d (square images)", W, H);
    MVE_CHECK(H % P == 0, MVE_ERR_ARG, "clip_patchify: H %d must be a multiple of P %d", H, P);
    MVE_CHECK(ld == (3 * P * P + 7) / 8 * 8, MVE_ERR_ARG, "clip_patchify: ld %d must be 3 * P * P rounded up to a multiple of 8 (%d)", ld, (3 * P * P + 7) / 8 * 8);
    MVE_CHECK((long long)B * 3 * H * W < (1ll << 31) && (long long)B * (H / P) * (H / P) * ld < (1ll << 31), MVE_ERR_ARG,
              "clip_patchify: batch B %d overflows 32-bit indexing", B);
    MVE_CHECK(aligned16(pixels) && aligned16(rows), MVE_ERR_ARG, "clip_patchify: d_pixels / d_rows must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_clip_patchify, pixels, rows, B, H, P, ld, (hipStream_t)stream);
}

extern "C" int mve_clip_vision_embed(int dtype, const void* patch, const void* cls, const void* pos, void* out, int B, int G2, int C, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "clip_vision_embed: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(patch && cls && pos && out, MVE_ERR_ARG, "clip_vision_embed: null pointer (d_patch / d_cls / d_pos / d_out)");
    MVE_CHECK(B >= 1 && G2 >= 1, MVE_ERR_ARG, "clip_vision_embed: bad B %d / G2 %d", B, G2);
    MVE_CHECK(C >= 8 && C % 8 == 0, MVE_ERR_ARG, "clip_vision_embed: C %d must be a multiple of 8", C);
    MVE_CHECK((long long)B * (G2 + 1) * C < (1ll << 31), MVE_ERR_ARG, "clip_vision_embed: batch B %d overflows 32-bit indexing", B);
    MVE_CHECK(aligned16(patch) && aligned16(cls) && aligned16(pos) && aligned16(out), MVE_ERR_ARG,
              "clip_vision_embed: d_patch / d_cls / d_pos / d_out must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_clip_vision_embed, patch, cls, pos, out, B, G2, C, (hipStream_t)stream);
}
