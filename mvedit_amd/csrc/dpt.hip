// DPT-hybrid primitives (include/mvedit_amd.h section 2e): the row kernels of the Omnidata normal predictor (the reference's
// `DPTDepthModel(backbone='vitb_rn50_384', num_channels=3)`, omnidata_modules/midas/dpt_depth.py:87-107, loaded at lib/apis/adapter3d.py:338-352)
// that the executor's GEMMs, convolutions, norms and attention do not already give: the operand rows of the ResNetV2 stem's 7 x 7 / 2
// convolution, its "same"-padded 3 x 3 / 2 max-pool, the stride-2 pixel gather in front of a stage's strided 1 x 1 shortcut, the x2 bilinear
// upsample with align_corners=True of the fusion blocks and the head, and (a + b) -> ReLU.  Everything else of the network is in
// csrc/builder_dpt.h.  All of them are bandwidth-bound row kernels over NHWC, one thread per 8 channels; written to be read, not tuned.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------------------
// stem rows: the 7 x 7 stride-2 convolution with TF "same" padding of an even-sized image (2 before, 3 after) as a GEMM.
// rows[(b*Ho + oy)*Ho + ox][(c, ky, kx)] = pixels[b][c][2*oy - 2 + ky][2*ox - 2 + kx] (0 outside), columns [147, ld) zero.
// pixels are NCHW: the (c, ky, kx) order is that of weight.reshape(Cout, 147).  One thread per 8 columns, element loads (3 channels).
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_dpt_stem_rows(const typename Tag::T* __restrict__ px, typename Tag::T* __restrict__ rows, int S, int Ho, int ld8,
                                                       long long total) {
    typedef typename Tag::T T;
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / ld8;
    const int k0 = (int)(i - row * ld8) * 8;
    const int b = (int)(row / ((long long)Ho * Ho)), g = (int)(row - (long long)b * Ho * Ho), oy = g / Ho, ox = g - oy * Ho;
    const T* img = px + (size_t)b * 3 * S * S;
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e;
        T v = (T)0.f;
        if (k < 147) {
            const int c = k / 49, r = k - c * 49, ky = r / 7, kx = r - ky * 7;
            const int y = 2 * oy - 2 + ky, x = 2 * ox - 2 + kx;
            if (y >= 0 && y < S && x >= 0 && x < S) v = img[((size_t)c * S + y) * S + x];
        }
        o[e] = v;
    }
    reinterpret_cast<V8*>(rows)[i] = o;
}

template <class Tag>
int launch_stem_rows(const void* px, void* rows, int B, int S, int ld, hipStream_t s) {
    typedef typename Tag::T T;
    const int Ho = S / 2;
    const long long total = (long long)B * Ho * Ho * (ld / 8);
    k_dpt_stem_rows<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>((const T*)px, (T*)rows, S, Ho, ld / 8, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// max-pool 3 x 3 / 2 with TF "same" padding of an even-sized map (0 before, 1 after): y[b, oy, ox, :] = max over x[b, 2oy + {0,1,2}, 2ox + {0,1,2}, :]
// with the taps outside the map left out.  transformers' BitMaxPool2d pads with 0 and timm's MaxPool2dSame with -inf; the input here is the
// output of a ReLU (>= 0), so a tap of 0 never wins against the in-range taps and the two are the same function.  Pure selection: exact.
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_dpt_maxpool(const typename Tag::T* __restrict__ x, typename Tag::T* __restrict__ y, int H, int W, int C8, long long total) {
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Ho = H / 2, Wo = W / 2;
    const long long pix = i / C8;
    const int c8 = (int)(i - pix * C8);
    const int b = (int)(pix / ((long long)Ho * Wo)), g = (int)(pix - (long long)b * Ho * Wo), oy = g / Wo, ox = g - oy * Wo;
    const V8* src = reinterpret_cast<const V8*>(x) + (size_t)b * H * W * C8 + c8;
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = 2 * oy + ky;
        if (yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = 2 * ox + kx;
            if (xx >= W) continue;
            const V8 v = src[((size_t)yy * W + xx) * C8];
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], Tag::to_f32(v[e]));
        }
    }
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = Tag::from_f32(m[e]);
    reinterpret_cast<V8*>(y)[i] = o;
}

template <class Tag>
int launch_maxpool(const void* x, void* y, int B, int H, int W, int C, hipStream_t s) {
    typedef typename Tag::T T;
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / 8);
    k_dpt_maxpool<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>((const T*)x, (T*)y, H, W, C / 8, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// stride-2 pixel gather: y[b, oy, ox, :] = x[b, 2oy, 2ox, :] -- the operand rows of a strided 1 x 1 convolution ("same" padding of a 1 x 1 / 2
// convolution over an even-sized map is no padding at all)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dpt_gather_s2(const u32x4* __restrict__ x, u32x4* __restrict__ y, int H, int W, int C8, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Ho = H / 2, Wo = W / 2;
    const long long pix = i / C8;
    const int c8 = (int)(i - pix * C8);
    const int b = (int)(pix / ((long long)Ho * Wo)), g = (int)(pix - (long long)b * Ho * Wo), oy = g / Wo, ox = g - oy * Wo;
    y[i] = x[(((size_t)b * H + 2 * oy) * W + 2 * ox) * C8 + c8];
}

// ---------------------------------------------------------------------------------------------------
// x2 bilinear upsample, align_corners=True (torch.nn.functional.interpolate's arithmetic: source coordinate = dst * (H - 1) / (2H - 1) in fp32,
// lambda1 = coordinate - floor, lambda0 = 1 - lambda1, rows combined as h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)); fp32, one rounding.
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_dpt_upsample2x(const typename Tag::T* __restrict__ x, typename Tag::T* __restrict__ y, int H, int W, int C8, float sy,
                                                        float sx, long long total) {
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Ho = 2 * H, Wo = 2 * W;
    const long long pix = i / C8;
    const int c8 = (int)(i - pix * C8);
    const int b = (int)(pix / ((long long)Ho * Wo)), g = (int)(pix - (long long)b * Ho * Wo), oy = g / Wo, ox = g - oy * Wo;
    const float fy = sy * (float)oy, fx = sx * (float)ox;
    int y0 = (int)fy, x0 = (int)fx;
    y0 = y0 > H - 1 ? H - 1 : y0; x0 = x0 > W - 1 ? W - 1 : x0;
    const int y1 = y0 < H - 1 ? y0 + 1 : y0, x1 = x0 < W - 1 ? x0 + 1 : x0;
    const float h1 = fy - (float)y0, h0 = 1.0f - h1, w1 = fx - (float)x0, w0 = 1.0f - w1;
    const V8* src = reinterpret_cast<const V8*>(x) + (size_t)b * H * W * C8 + c8;
    const V8 a = src[((size_t)y0 * W + x0) * C8], bq = src[((size_t)y0 * W + x1) * C8], c = src[((size_t)y1 * W + x0) * C8], d = src[((size_t)y1 * W + x1) * C8];
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        o[e] = Tag::from_f32(h0 * (w0 * Tag::to_f32(a[e]) + w1 * Tag::to_f32(bq[e])) + h1 * (w0 * Tag::to_f32(c[e]) + w1 * Tag::to_f32(d[e])));
    reinterpret_cast<V8*>(y)[i] = o;
}

template <class Tag>
int launch_upsample2x(const void* x, void* y, int B, int H, int W, int C, hipStream_t s) {
    typedef typename Tag::T T;
    const long long total = (long long)B * 4 * H * W * (C / 8);
    const float sy = H > 1 ? (float)(H - 1) / (float)(2 * H - 1) : 0.f, sx = W > 1 ? (float)(W - 1) / (float)(2 * W - 1) : 0.f;
    k_dpt_upsample2x<Tag><<<mve_cdiv(total, 256), 256, 0, s>>>((const T*)x, (T*)y, H, W, C / 8, sy, sx, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

// ---------------------------------------------------------------------------------------------------
// y = max(a + b, 0) (b may be null: plain ReLU); the sum in fp32, one rounding.  n8 vectors of 8 elements.
// ---------------------------------------------------------------------------------------------------
template <class Tag>
__global__ __launch_bounds__(256) void k_dpt_add_relu(const typename Tag::V8* __restrict__ a, const typename Tag::V8* __restrict__ b, typename Tag::V8* __restrict__ y,
                                                      long long n8) {
    typedef typename Tag::V8 V8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const V8 va = a[i];
    V8 o;
    if (b) {
        const V8 vb = b[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = Tag::from_f32(fmaxf(Tag::to_f32(va[e]) + Tag::to_f32(vb[e]), 0.f));
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = Tag::from_f32(fmaxf(Tag::to_f32(va[e]), 0.f));
    }
    y[i] = o;
}

template <class Tag>
int launch_add_relu(const void* a, const void* b, void* y, size_t n, hipStream_t s) {
    typedef typename Tag::V8 V8;
    k_dpt_add_relu<Tag><<<mve_cdiv(n / 8, 256), 256, 0, s>>>((const V8*)a, (const V8*)b, (V8*)y, (long long)(n / 8));
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// shared argument checks of the NHWC kernels: 16-bit dtype, non-null aligned pointers, C % 8 == 0, 32-bit indexable tensors
int check_nhwc(const char* who, int dtype, const void* x, const void* y, int B, int H, int W, int C, long long out_pixels_per_image) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "%s: dtype %d must be f16 or bf16", who, dtype);
    MVE_CHECK(x && y, MVE_ERR_ARG, "%s: null pointer (d_x / d_y)", who);
    MVE_CHECK(B >= 1 && H >= 1 && W >= 1, MVE_ERR_ARG, "%s: bad B %d / H %d / W %d", who, B, H, W);
    MVE_CHECK(C >= 8 && C % 8 == 0, MVE_ERR_ARG, "%s: C %d must be a multiple of 8", who, C);
    MVE_CHECK((long long)B * H * W * C < (1ll << 31) && (long long)B * out_pixels_per_image * C < (1ll << 31), MVE_ERR_ARG, "%s: batch B %d overflows 32-bit indexing", who, B);
    MVE_CHECK(aligned16(x) && aligned16(y), MVE_ERR_ARG, "%s: d_x / d_y must be 16-byte aligned", who);
    return MVE_OK;
}

}  // namespace

extern "C" int mve_dpt_stem_rows(int dtype, const void* pixels, int B, int S, void* rows, int ld, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "dpt_stem_rows: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(pixels && rows, MVE_ERR_ARG, "dpt_stem_rows: null pointer (d_pixels / d_rows)");
    MVE_CHECK(B >= 1 && S >= 2 && S % 2 == 0, MVE_ERR_ARG, "dpt_stem_rows: bad B %d / S %d (S must be even)", B, S);
    MVE_CHECK(ld == 152, MVE_ERR_ARG, "dpt_stem_rows: ld %d must be 152 (3 * 7 * 7 = 147 rounded up to a multiple of 8)", ld);
    MVE_CHECK((long long)B * 3 * S * S < (1ll << 31) && (long long)B * (S / 2) * (S / 2) * ld < (1ll << 31), MVE_ERR_ARG, "dpt_stem_rows: batch B %d overflows 32-bit indexing", B);
    MVE_CHECK(aligned16(rows), MVE_ERR_ARG, "dpt_stem_rows: d_rows must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_stem_rows, pixels, rows, B, S, ld, (hipStream_t)stream);
}

extern "C" int mve_dpt_maxpool(int dtype, const void* x, int B, int H, int W, int C, void* y, void* stream) {
    const int rc = check_nhwc("dpt_maxpool", dtype, x, y, B, H, W, C, (long long)(H / 2) * (W / 2));
    if (rc) return rc;
    MVE_CHECK(H % 2 == 0 && W % 2 == 0, MVE_ERR_ARG, "dpt_maxpool: H %d and W %d must be even (\"same\" padding of an even map: 0 before, 1 after)", H, W);
    return MVE_DISPATCH_16(dtype, launch_maxpool, x, y, B, H, W, C, (hipStream_t)stream);
}

extern "C" int mve_dpt_gather_s2(int dtype, const void* x, int B, int H, int W, int C, void* y, void* stream) {
    const int rc = check_nhwc("dpt_gather_s2", dtype, x, y, B, H, W, C, (long long)(H / 2) * (W / 2));
    if (rc) return rc;
    MVE_CHECK(H % 2 == 0 && W % 2 == 0, MVE_ERR_ARG, "dpt_gather_s2: H %d and W %d must be even", H, W);
    const long long total = (long long)B * (H / 2) * (W / 2) * (C / 8);
    k_dpt_gather_s2<<<mve_cdiv(total, 256), 256, 0, (hipStream_t)stream>>>((const u32x4*)x, (u32x4*)y, H, W, C / 8, total);
    MVE_LAUNCH_CHECK();
    return MVE_OK;
}

extern "C" int mve_dpt_upsample2x(int dtype, const void* x, int B, int H, int W, int C, void* y, void* stream) {
    const int rc = check_nhwc("dpt_upsample2x", dtype, x, y, B, H, W, C, 4ll * H * W);
    if (rc) return rc;
    return MVE_DISPATCH_16(dtype, launch_upsample2x, x, y, B, H, W, C, (hipStream_t)stream);
}

extern "C" int mve_dpt_add_relu(int dtype, const void* a, const void* b, void* y, size_t n, void* stream) {
    MVE_CHECK(dtype == MVE_F16 || dtype == MVE_BF16, MVE_ERR_ARG, "dpt_add_relu: dtype %d must be f16 or bf16", dtype);
    MVE_CHECK(a && y, MVE_ERR_ARG, "dpt_add_relu: null pointer (d_a / d_y)");
    MVE_CHECK(n >= 8 && n % 8 == 0, MVE_ERR_ARG, "dpt_add_relu: n %zu must be a multiple of 8", n);
    MVE_CHECK(aligned16(a) && aligned16(b) && aligned16(y), MVE_ERR_ARG, "dpt_add_relu: d_a / d_b / d_y must be 16-byte aligned");
    return MVE_DISPATCH_16(dtype, launch_add_relu, a, b, y, n, (hipStream_t)stream);
}
