// The index arithmetic of bilinear(align_corners=True) upsampling, shared by everything that works on an upsampled map without building
// it: the segmentation terms (upsample_ce / ohem / lovasz / rmi), the test-phase fusions (ms_eval / crop_eval) and the adjoint of the
// exchange units (cseg_bilinear.h). torch's own fp32 index arithmetic, so the taps (i0, i1) are torch's. The weight l1 = f - (float)i0
// with f = s * (float)o has two legal roundings: from the rounded product (a host build, torch on the CPU) or, when the compiler
// contracts the product into the subtraction (hipcc's default for gfx950: v_mul, v_cvt, then v_fma l1 = s*o - i0), from the exact one.
// They differ by up to half an ulp of f (1.5e-5 at column 260). The exchange kernels -- bl_tap here, the forward copies in upcat.hip and
// fuse.hip -- leave that choice to the compiler, instance by instance, and their tests accept exactly these two weights
// (tests/exchange_cases.py); cseg_ms_fuse.h pins it for the test-phase kernel. DESIGN.md section 26 says what lives here and what must
// not: indices, adjoint weights, loop nests -- never the value blends.
#pragma once
#include "cseg_common.h"

// output index o -> lower / upper input tap and the weight of the upper one
__device__ __forceinline__ void bl_tap(float s, int n_in, int o, int& i0, int& i1, float& l1) {
    const float f = s * (float)o;
    i0 = (int)f;
    i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
    l1 = f - (float)i0;
}

// the lower tap alone; host side too: the launchers count label pixels per tap with the device's own arithmetic
__host__ __device__ __forceinline__ int tap0(float s, int o) { return (int)(s * (float)o); }

// smallest o in [0, n_out] with tap0(s, o) >= c (n_out when there is none); tap0 is monotone in o
__host__ __device__ __forceinline__ int first_with_tap(float s, int n_out, int c) {
    if (c <= 0) return 0;
    if (!(s > 0.f)) return n_out;
    int o = (int)((float)c / s);
    if (o > n_out) o = n_out;
    if (o < 0) o = 0;
    while (o > 0 && tap0(s, o - 1) >= c) --o;
    while (o < n_out && tap0(s, o) < c) ++o;
    return o;
}

// first / last fine index whose lower tap i0 lies in [c_lo - 1, c_hi]  (c_lo..c_hi coarse indices, inclusive)
__device__ __forceinline__ void bl_fine_range(float s, int n_fine, int c_lo, int c_hi, int& lo, int& hi) {
    lo = 0; hi = n_fine - 1;
    if (s > 0.f) {
        lo = max(0, (int)ceilf((float)(c_lo - 1) / s) - 1);
        while (lo < n_fine - 1 && (int)(s * (float)lo) < c_lo - 1) ++lo;
        hi = min(n_fine - 1, (int)floorf((float)(c_hi + 1) / s) + 1);
        while (hi > 0 && (int)(s * (float)hi) > c_hi) --hi;
    }
}

// weight with which the fine index of taps (i0, i1, l1) lands on the coarse index c: the transpose of the forward's two taps (both
// on c at the far edge, where i1 == i0)
__device__ __forceinline__ float bl_adjoint_weight(int i0, int i1, float l1, int c) {
    float wt = 0.f;
    if (i0 == c) wt += 1.f - l1;
    if (i1 == c) wt += l1;
    return wt;
}

// Exact adjoint in gather form, for one coarse element (ys, xs) of an h x w map upsampled to H x W: the sum over the fine pixels (Y, X)
// whose taps touch it of wy * wx * value, rows first. f(Y, X, y0, y1, ly1, x0, x1, lx1, v) sets the pixel's value v and returns true,
// or returns false for a pixel that takes no part (skipped, which is not the same bits as adding 0).
template <class F>
__device__ __forceinline__ float bl_gather_adjoint(float sy, float sx, int h, int w, int H, int W, int ys, int xs, F f) {
    int y_lo, y_hi, x_lo, x_hi;
    bl_fine_range(sy, H, ys, ys, y_lo, y_hi);
    bl_fine_range(sx, W, xs, xs, x_lo, x_hi);
    float acc = 0.f;
    for (int Y = y_lo; Y <= y_hi; ++Y) {
        int y0, y1;
        float ly1;
        bl_tap(sy, h, Y, y0, y1, ly1);
        const float wy = bl_adjoint_weight(y0, y1, ly1, ys);
        if (wy == 0.f) continue;
        float racc = 0.f;
        for (int X = x_lo; X <= x_hi; ++X) {
            int x0, x1;
            float lx1, v;
            bl_tap(sx, w, X, x0, x1, lx1);
            const float wx = bl_adjoint_weight(x0, x1, lx1, xs);
            if (wx == 0.f) continue;
            if (f(Y, X, y0, y1, ly1, x0, x1, lx1, v)) racc += wx * v;
        }
        acc += wy * racc;
    }
    return acc;
}

// Extents and scales of a term on [B,K,h,w] logits and [B,H,W] labels; a term extends it with what only it needs.
struct UpDims {
    int B, K, h, w, H, W;
    float sy, sx;
};

// the two refusals every term makes, under the caller's name
static inline int up_dims(const char* what, UpDims* d, int B, int K, int h, int w, int H, int W) {
    CSEG_REQUIRE(B > 0 && K > 0 && h > 0 && w > 0 && H > 0 && W > 0, "%s: empty shape", what);
    CSEG_REQUIRE(H >= h && W >= w, "%s: only upsampling is supported (%dx%d -> %dx%d)", what, h, w, H, W);
    d->B = B; d->K = K; d->h = h; d->w = w; d->H = H; d->W = W;
    d->sy = ac_scale(h, H); d->sx = ac_scale(w, W);
    return 1;
}
