// Test phase: sliding-crop evaluation (sscrop_test / mscrop_test) fused with the flip, the scale sum and the argmax.
// Reference: segmentor/tester.py:351-378 (sscrop_test: resize the input to the canvas, run the net on crop-sized tiles whose starts
// come from _decide_intersection, upsample every tile's coarse output to the crop, add it into a [B,K,hs,ws] logits canvas and a
// count canvas, divide, resize the canvas back to the input size) and :505-523 (mscrop_test: per scale, ss_test below 1 and
// sscrop_test from 1 on, probs = P(x) + flip(P(flip(x))), full_probs += probs), followed by the argmax of :189. At 19 x 2048 x 4096
// each of the two canvases is 637 MB per image and the reference makes about a dozen passes over them. Everything between the coarse
// crop outputs and the argmax is linear, so here neither canvas exists: one kernel reads the coarse per-crop maps and writes one
// byte per pixel.
//
// Per output pixel (y,x), class and term the kernel evaluates the nested form
//     the bilinear taps of (y,x) in the canvas  ->  per canvas tap the one or two covering tiles per axis  ->  per tile the bilinear
//     taps in its coarse map  ->  the tile sum in the reference's (height-major) tile order  ->  the division by the count (1, 2 or 4:
//     exact)  ->  the canvas blend  ->  + the mirrored input's stack evaluated at the MIRRORED output column W-1-x, which tiles the
//     mirrored canvas (with ragged sizes its overlap band is on the other side)  ->  the term sum in scale_search order
// with a running (best, index) pair; strict '>' keeps the first index among equal maxima. A plain term (ss_test of a scale below 1)
// is the same form with canvas = crop = output size and one tile: its canvas blend factors are 0 and what is left is ms_fuse_kernel's
// expression, bit for bit. A canvas tap whose blend factor is exactly 0 is not read (its product is 0 for finite logits), so a
// scale-1 canvas and plain terms cost one tap, not four.
//
// crop_fuse_kernel   a block owns an 8 x 32 patch of output pixels. All tap data depend on y alone or on x alone: per term the block
//                    computes them once for its 8 rows, 32 columns and 32 mirrored columns into LDS (tile starts from (hs, ws, ch, cw)
//                    inside the kernel: start(i) = min(i * crop, total - crop)), with the package's fp32 index arithmetic (bl_tap;
//                    DESIGN.md section 26) on both levels. Classes run in the outer loop, terms inside. Floating-point contraction is off, every
//                    rounding is where the source puts it. No atomics: deterministic.
#include "cseg_taps.h"

#pragma clang fp contract(off)

namespace {

constexpr int CROP_MAX_TERMS = 8;        // MS_MAX_TERMS of ms_eval.hip
constexpr int CROP_MAX_K = 256;
constexpr int CROP_TY = 8, CROP_TX = 32;
constexpr int CROP_NO = CROP_TY + 2 * CROP_TX;      // axis entries of a block: rows, columns, mirrored columns

struct CropTerm {
    const float* a;      // [ny*nx,B,K,hc,wc] coarse crop maps in tile order (height-major), or null
    const float* b;      // the same for the mirrored input, or null
    int hs, ws;          // canvas
    int ch, cw;          // crop
    int hc, wc;          // coarse map of one crop
    int ny, nx;          // tiles
    float sy, sx;        // canvas <- output
    float ty, tx;        // coarse map <- crop
};

struct CropArgs {
    CropTerm t[CROP_MAX_TERMS];
    int n, B, K, H, W;
};

// One canvas row (or column) seen from the tiles that cover it: slot a always, slot b when a second tile covers it (else -1).
// a / b = (element offset of the tile and of the lower coarse tap within a [B,K,hc,wc] stack) * 2 + (the upper tap is one further);
// la / lb = the coarse blend factor.
struct alignas(16) AxisTap {
    int a, b;
    float la, lb;
};

__device__ __forceinline__ int crop_pack(float s, int n_coarse, int local, int stride, int tile_off, float& l) {
    int i0, i1;
    bl_tap(s, n_coarse, local, i0, i1, l);
    // as in ms_fuse_kernel: these change no tap, they make every address provably inside the plane
    i0 = min(i0, n_coarse - 1); i1 = min(i1, n_coarse - 1);
    return ((tile_off + i0 * stride) << 1) | (i1 != i0 ? 1 : 0);
}

// P: canvas index in [0, total); crop <= total; nt = ceil(total / crop) tiles with start(i) = min(i * crop, total - crop)
__device__ __forceinline__ AxisTap crop_axis_tap(int P, int total, int crop, int nt, float s, int n_coarse, int stride, int tile_stride) {
    AxisTap e;
    e.b = -1; e.lb = 0.f;
    const int last = total - crop;           // start of the last tile
    const int t0 = P / crop;
    if (t0 >= nt - 1) {
        e.a = crop_pack(s, n_coarse, P - last, stride, (nt - 1) * tile_stride, e.la);
    } else {
        e.a = crop_pack(s, n_coarse, P - t0 * crop, stride, t0 * tile_stride, e.la);
        if (P >= last) e.b = crop_pack(s, n_coarse, P - last, stride, (nt - 1) * tile_stride, e.lb);    // then t0 == nt - 2
    }
    return e;
}

// bilinear(align_corners=True) value of one tile's coarse map: vertical blend first, one fused multiply-add across the columns
__device__ __forceinline__ float crop_u(const float* __restrict__ s, int wc, int p, float ly1, int q, float lx) {
    const int r0 = p >> 1, r1 = r0 + (p & 1) * wc;
    const int x0 = q >> 1, x1 = x0 + (q & 1);
    const float ly0 = 1.f - ly1;
    const float c0 = ly0 * s[r0 + x0] + ly1 * s[r1 + x0];
    const float c1 = ly0 * s[r0 + x1] + ly1 * s[r1 + x1];
    return fmaf(lx, c1 - c0, c0);
}

// one canvas element: ((0 + U_1) + U_2) + ... over the covering tiles in tile order, divided by their number
__device__ __forceinline__ float crop_canvas(const float* __restrict__ s, int wc, const AxisTap& r, const AxisTap& c) {
    float v = crop_u(s, wc, r.a, r.la, c.a, c.la);
    float inv = 1.f;
    if (c.b >= 0) { v = v + crop_u(s, wc, r.a, r.la, c.b, c.lb); inv = 0.5f; }
    if (r.b >= 0) {
        v = v + crop_u(s, wc, r.b, r.lb, c.a, c.la);
        if (c.b >= 0) v = v + crop_u(s, wc, r.b, r.lb, c.b, c.lb);
        inv = inv * 0.5f;
    }
    return v * inv;
}

// grid = (ceil(W / 32), ceil(H / 8), B)
__global__ __launch_bounds__(256) void crop_fuse_kernel(CropArgs A, uint8_t* __restrict__ pred, float* __restrict__ fused) {
    __shared__ AxisTap taps[2][CROP_MAX_TERMS][CROP_NO];
    __shared__ float blend[CROP_MAX_TERMS][CROP_NO];
    const int tid = threadIdx.x, lx = tid & (CROP_TX - 1), ly = tid / CROP_TX;
    const int x_lo = blockIdx.x * CROP_TX, y_lo = blockIdx.y * CROP_TY, b = blockIdx.z;
    const size_t BK = (size_t)A.B * A.K;

    if (tid < CROP_NO) {
        const int o = tid;
        const bool row = o < CROP_TY;
        int coord;      // rows / columns beyond the image repeat the last one: nobody reads them
        if (row) coord = min(y_lo + o, A.H - 1);
        else if (o < CROP_TY + CROP_TX) coord = min(x_lo + o - CROP_TY, A.W - 1);
        else coord = A.W - 1 - min(x_lo + o - CROP_TY - CROP_TX, A.W - 1);
        for (int i = 0; i < A.n; ++i) {
            const CropTerm& t = A.t[i];
            const int plane = t.hc * t.wc;
            const int total = row ? t.hs : t.ws, crop = row ? t.ch : t.cw, nt = row ? t.ny : t.nx;
            const int n_coarse = row ? t.hc : t.wc, stride = row ? t.wc : 1;
            const int tile_stride = (int)BK * plane * (row ? t.nx : 1);
            int P0, P1;
            float L;
            bl_tap(row ? t.sy : t.sx, total, coord, P0, P1, L);
            P0 = min(P0, total - 1); P1 = min(P1, total - 1);
            blend[i][o] = L;
            taps[0][i][o] = crop_axis_tap(P0, total, crop, nt, row ? t.ty : t.tx, n_coarse, stride, tile_stride);
            taps[1][i][o] = crop_axis_tap(P1, total, crop, nt, row ? t.ty : t.tx, n_coarse, stride, tile_stride);
        }
    }
    __syncthreads();

    const int y = y_lo + ly, x = x_lo + lx;
    if (y >= A.H || x >= A.W) return;
    const size_t HW = (size_t)A.H * A.W;
    const size_t p = (size_t)y * A.W + x;
    const int ro = ly, co[2] = {CROP_TY + lx, CROP_TY + CROP_TX + lx};

    float best = 0.f;
    int best_k = 0;
    for (int k = 0; k < A.K; ++k) {
        float v = 0.f;
        for (int i = 0; i < A.n; ++i) {
            const CropTerm& t = A.t[i];
            const size_t plane = ((size_t)b * A.K + k) * ((size_t)t.hc * t.wc);
            const float LY = blend[i][ro];
            const AxisTap r0 = taps[0][i][ro], r1 = taps[1][i][ro];
            float u = 0.f;
#pragma unroll
            for (int m = 0; m < 2; ++m) {          // the plain stack at column x, the mirrored input's stack at column W-1-x
                const float* base = m ? t.b : t.a;
                if (!base) continue;
                const float* s = base + plane;
                const float LX = blend[i][co[m]];
                const AxisTap c0 = taps[0][i][co[m]];
                float e0 = crop_canvas(s, t.wc, r0, c0);
                if (LY != 0.f) e0 = (1.f - LY) * e0 + LY * crop_canvas(s, t.wc, r1, c0);
                float um = e0;
                if (LX != 0.f) {
                    const AxisTap c1 = taps[1][i][co[m]];
                    float e1 = crop_canvas(s, t.wc, r0, c1);
                    if (LY != 0.f) e1 = (1.f - LY) * e1 + LY * crop_canvas(s, t.wc, r1, c1);
                    um = fmaf(LX, e1 - e0, e0);
                }
                u = (m && t.a) ? u + um : um;
            }
            v = v + u;
        }
        if (fused) fused[((size_t)b * A.K + k) * HW + p] = v;
        if (k == 0 || v > best) { best = v; best_k = k; }
    }
    if (pred) pred[(size_t)b * HW + p] = (uint8_t)best_k;
}

}  // namespace

extern "C" int cseg_crop_fuse_argmax(int n_terms, const float* const* plain, const float* const* flipped, const int* dims, int B,
                                     int K, int H, int W, uint8_t* pred, float* fused, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(n_terms >= 1 && n_terms <= CROP_MAX_TERMS, "crop_fuse_argmax: %d terms (1 to %d are supported)", n_terms,
                 CROP_MAX_TERMS);
    CSEG_REQUIRE(dims && (plain || flipped), "crop_fuse_argmax: null term arrays");
    CSEG_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0, "crop_fuse_argmax: empty shape");
    CSEG_REQUIRE(K <= CROP_MAX_K, "crop_fuse_argmax: %d classes (the prediction is one byte; at most %d)", K, CROP_MAX_K);
    CSEG_REQUIRE(pred || fused, "crop_fuse_argmax: both outputs are null");
    CSEG_REQUIRE((long)B * H * W < 2147483647L && B <= 65535 && (H + CROP_TY - 1) / CROP_TY <= 65535,
                 "crop_fuse_argmax: %d x %d x %d output pixels are too many for one launch", B, H, W);
    CropArgs A;
    A.n = n_terms; A.B = B; A.K = K; A.H = H; A.W = W;
    for (int i = 0; i < CROP_MAX_TERMS; ++i) {
        CropTerm& t = A.t[i];
        t.a = nullptr; t.b = nullptr;
        t.hs = t.ws = t.ch = t.cw = t.hc = t.wc = t.ny = t.nx = 1;
        t.sy = t.sx = t.ty = t.tx = 0.f;
        if (i >= n_terms) continue;
        const int* d = dims + (size_t)i * CSEG_CROP_TERM_INTS;
        const bool tiled = d[0] != 0 || d[1] != 0 || d[2] != 0 || d[3] != 0;
        t.hs = tiled ? d[0] : H; t.ws = tiled ? d[1] : W;
        t.ch = tiled ? d[2] : H; t.cw = tiled ? d[3] : W;
        t.hc = d[4]; t.wc = d[5];
        CSEG_REQUIRE(t.hs > 0 && t.ws > 0 && t.ch > 0 && t.cw > 0 && t.hc > 0 && t.wc > 0,
                     "crop_fuse_argmax: term %d is empty (canvas %d x %d, crop %d x %d, coarse map %d x %d)", i, t.hs, t.ws, t.ch, t.cw,
                     t.hc, t.wc);
        t.a = plain ? plain[i] : nullptr;
        t.b = flipped ? flipped[i] : nullptr;
        CSEG_REQUIRE(t.a || t.b, "crop_fuse_argmax: term %d has neither a plain nor a flipped map", i);
        CSEG_REQUIRE(t.hs >= t.ch && t.ws >= t.cw, "crop_fuse_argmax: term %d: the canvas %d x %d is smaller than the crop %d x %d", i,
                     t.hs, t.ws, t.ch, t.cw);
        t.ny = (t.hs + t.ch - 1) / t.ch; t.nx = (t.ws + t.cw - 1) / t.cw;
        CSEG_REQUIRE(!tiled || d[6] == t.ny * t.nx,
                     "crop_fuse_argmax: term %d: a stack of %d tiles for the %d x %d tiles of a %d x %d canvas under a %d x %d crop", i,
                     d[6], t.ny, t.nx, t.hs, t.ws, t.ch, t.cw);
        CSEG_REQUIRE((double)t.ny * t.nx * B * K * t.hc * t.wc < 1073741824.0,
                     "crop_fuse_argmax: term %d is too large (%d x %d tiles of %d x %d x %d x %d; fewer than 2^30 elements are supported)",
                     i, t.ny, t.nx, B, K, t.hc, t.wc);
        t.sy = ac_scale(t.hs, H); t.sx = ac_scale(t.ws, W);
        t.ty = ac_scale(t.hc, t.ch); t.tx = ac_scale(t.wc, t.cw);
    }
    const dim3 grid((unsigned)((W + CROP_TX - 1) / CROP_TX), (unsigned)((H + CROP_TY - 1) / CROP_TY), (unsigned)B);
    hipLaunchKernelGGL(crop_fuse_kernel, grid, dim3(256), 0, stream, A, pred, fused);
    CSEG_CHECK_LAUNCH("crop_fuse_kernel");
    return 1;
}
