// Validation scoring on the reference's resize: cv2's float INTER_CUBIC of the coarse logits with the argmax, one kernel.
// Reference: segmentor/tools/evaluator/standard.py:75-103 (per image: logits[:border_h, :border_w] -> cv2.resize(..., ori_img_size,
// INTER_CUBIC) on the host -> argmax -> score against the label file at its own size) and, for the mirrored pair of the LIP pass,
// segmentor/trainer_contrastive.py:335-346 ((outputs + flip(swap(outputs_rev))) / 2. at coarse size, ahead of the resize). Here the
// [B,K,H,W] map never exists and nothing goes to the host: the kernels read the coarse maps and write one byte per pixel.
//
// The rule is cv2's scalar source (modules/imgproc/src/resize.cpp: the xofs / alpha table loop, interpolateCubic, HResizeCubic,
// VResizeCubic), fp32 with every product and sum rounded on its own:
//   scale = 1.0 / ((double)dst / (double)crop)                       host, double
//   f = (float)(((double)x + 0.5) * scale - 0.5);  s = floor(f);  t = f - (float)s;      not clamped
//   coefficients: cubic_coeffs_f32(t) (cseg_cubic.h), A = -0.75
//   taps: clamp(s - 1 + j, 0, crop - 1), j = 0..3 (replicated border; the crop bounds the clamp, not the map)
//   source value: a[b,k,r,c], or with a mirrored operand (a[b,k,r,c] + bm[b,perm[k],r,w-1-c]) / 2.f -- mirrored over the map's
//   full width w
//   horizontal pass per tap row: hz = ((s0*c0 + s1*c1) + s2*c2) + s3*c3;  vertical pass: v = ((hz0*d0 + hz1*d1) + hz2*d2) + hz3*d3
//   pred = first index among equal maxima (strict '>').
//
// cubic_direct_kernel  one thread per output pixel: 4 column indices, 4 row offsets and 8 coefficients once, ahead of the class
//                      loop; 16 taps per class (32 with a mirrored operand) straight from global memory. No LDS, no barrier, every
//                      geometry.
// cubic_tiled_kernel   separable through static LDS, for upsampling by at least 2 in both axes. A 256-thread block owns a 32 x 64
//                      output tile, 8 pixels per thread (one column, 8 consecutive rows). Per class: the tile's source footprint
//                      (at most 20 x 36 values; 11 x 19 at 4x) is staged with the mirrored average applied, the horizontal pass
//                      goes into a second array (footprint rows x 64 columns), then every thread does the vertical pass of its 8
//                      pixels. Two barriers per class; no thread returns ahead of one; threads beyond the image edge compute and
//                      store nothing. The footprint comes from the same floor(f) statements as the taps, so it covers them exactly.
// Both execute the same per-value statements in the same order (cubic_value, cubic_dot), so they are bit-identical. No atomics.
#include "cseg_cubic.h"
#include "cseg_ms_fuse.h"        // MsPerm, ms_perm_fault, MS_MAX_K

namespace {

constexpr int CB_TILE_H = 32, CB_TILE_W = 64;
constexpr int CB_ROWS_PER_THREAD = CB_TILE_H / 4;                        // four waves, each 8 rows of the tile
constexpr int CB_FOOT_H = CB_TILE_H / 2 + 4;                             // footprint of a tile at a scale factor >= 2: 20 x 36
constexpr int CB_FOOT_W = CB_TILE_W / 2 + 4;
constexpr int CB_STAGE = (CB_FOOT_H * CB_FOOT_W + 255) / 256;            // staged values per thread and class: 3
constexpr int CB_HZ_ROWS = (CB_FOOT_H + 3) / 4;                          // horizontal-pass rows per thread and class: 5

struct CubicArgs {
    const float* a;      // [B,K,h,w]
    const float* b;      // [B,K,h,w] mirrored operand, or null
    int B, K, h, w, ch, cw, H, W;
    double sy, sx;       // 1.0 / ((double)H / ch), 1.0 / ((double)W / cw)
    int permuted;
    MsPerm perm;
};

// cv2's destination -> source coordinate for one axis: the double product and the difference each rounded on their own, the float
// floor, the fp32 fraction. Neither is clamped for cubic.
__device__ __forceinline__ void cubic_src(int x, double scale, int& s, float& t) {
#pragma clang fp contract(off)
    const double p = ((double)x + 0.5) * scale;
    const float f = (float)(p - 0.5);
    const float fl = floorf(f);
    s = (int)fl;
    t = f - fl;
}

__device__ __forceinline__ int cubic_clamp(int i, int n) { return min(max(i, 0), n - 1); }

// the value the resize reads at (r, c): off = r * w + c, offm = r * w + (w - 1 - c)
__device__ __forceinline__ float cubic_value(const float* __restrict__ pa, const float* __restrict__ pb, int off, int offm) {
#pragma clang fp contract(off)
    const float v = pa[off];
    return pb ? (v + pb[offm]) / 2.f : v;
}

__device__ __forceinline__ float cubic_dot(float s0, float s1, float s2, float s3, const float (&c)[4]) {
    return f_add(f_add(f_add(f_mul(s0, c[0]), f_mul(s1, c[1])), f_mul(s2, c[2])), f_mul(s3, c[3]));
}

__global__ __launch_bounds__(256) void cubic_direct_kernel(CubicArgs A, uint8_t* __restrict__ pred, float* __restrict__ fused) {
#pragma clang fp contract(off)
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long HW = (long)A.H * A.W;
    if (g >= (long)A.B * HW) return;
    const int b = (int)(g / HW);
    const int p = (int)(g - (long)b * HW);
    const int y = p / A.W, x = p - y * A.W;

    int sy, sx;
    float ty, tx, cy[4], cx[4];
    cubic_src(y, A.sy, sy, ty);
    cubic_src(x, A.sx, sx, tx);
    cubic_coeffs_f32(ty, cy);
    cubic_coeffs_f32(tx, cx);
    int ro[4], co[4], cm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ro[j] = cubic_clamp(sy - 1 + j, A.ch) * A.w;
        co[j] = cubic_clamp(sx - 1 + j, A.cw);
        cm[j] = A.w - 1 - co[j];
    }

    const size_t plane = (size_t)A.h * A.w;
    float best = 0.f;
    int best_k = 0;
    for (int k = 0; k < A.K; ++k) {
        const float* pa = A.a + ((size_t)b * A.K + k) * plane;
        const float* pb = A.b ? A.b + ((size_t)b * A.K + (A.permuted ? A.perm.get(k) : k)) * plane : nullptr;
        float hz[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            hz[r] = cubic_dot(cubic_value(pa, pb, ro[r] + co[0], ro[r] + cm[0]), cubic_value(pa, pb, ro[r] + co[1], ro[r] + cm[1]),
                              cubic_value(pa, pb, ro[r] + co[2], ro[r] + cm[2]), cubic_value(pa, pb, ro[r] + co[3], ro[r] + cm[3]), cx);
        const float v = cubic_dot(hz[0], hz[1], hz[2], hz[3], cy);
        if (fused) fused[((size_t)b * A.K + k) * HW + p] = v;
        if (k == 0 || v > best) { best = v; best_k = k; }
    }
    if (pred) pred[g] = (uint8_t)best_k;
}

// grid: B * tiles_y * tiles_x blocks, the tile column fastest
__global__ __launch_bounds__(256) void cubic_tiled_kernel(CubicArgs A, int tiles_y, int tiles_x, uint8_t* __restrict__ pred,
                                                          float* __restrict__ fused) {
#pragma clang fp contract(off)
    __shared__ float stage[CB_FOOT_H * CB_FOOT_W];
    __shared__ float hzb[CB_FOOT_H * CB_TILE_W];
    const int tid = threadIdx.x, xl = tid & 63, wv = tid >> 6;
    const int tile = (int)blockIdx.x;
    const int b = tile / (tiles_y * tiles_x);
    const int ty_ = (tile - b * tiles_y * tiles_x) / tiles_x;
    const int tx_ = tile - (b * tiles_y + ty_) * tiles_x;
    const int y0 = ty_ * CB_TILE_H, x0 = tx_ * CB_TILE_W;

    // The footprint: floor(f) is monotone in the destination index and so is the clamp, so the taps of every pixel of the tile lie
    // between the first tap of its first row / column and the last tap of its last. The launcher admits scale factors >= 2 only,
    // for which the extent is at most CB_FOOT_H x CB_FOOT_W (a destination step is at most half a source step: 31 / 2 and 63 / 2
    // between the floors, four taps on top); the min() and the second clamps below never bind then, and keep every LDS index
    // inside the arrays by construction.
    int s_lo, s_hi;
    float unused;
    cubic_src(y0, A.sy, s_lo, unused);
    cubic_src(min(y0 + CB_TILE_H, A.H) - 1, A.sy, s_hi, unused);
    const int row_lo = cubic_clamp(s_lo - 1, A.ch);
    const int nrows = min(cubic_clamp(s_hi + 2, A.ch) - row_lo + 1, CB_FOOT_H);
    cubic_src(x0, A.sx, s_lo, unused);
    cubic_src(min(x0 + CB_TILE_W, A.W) - 1, A.sx, s_hi, unused);
    const int col_lo = cubic_clamp(s_lo - 1, A.cw);
    const int ncols = min(cubic_clamp(s_hi + 2, A.cw) - col_lo + 1, CB_FOOT_W);

    // staging: value e of the footprint (row-major) is this thread's for e = tid + 256 q
    int st_off[CB_STAGE], st_offm[CB_STAGE], st_lds[CB_STAGE];
#pragma unroll
    for (int q = 0; q < CB_STAGE; ++q) {
        const int e = tid + 256 * q;
        const int r = e / ncols, c = e - r * ncols;
        st_off[q] = e < nrows * ncols ? (row_lo + r) * A.w + (col_lo + c) : -1;
        st_offm[q] = (row_lo + r) * A.w + (A.w - 1 - (col_lo + c));
        st_lds[q] = r * CB_FOOT_W + c;
    }

    // horizontal pass: this thread's column of the tile, rows wv, wv + 4, ... of the footprint
    const int x = x0 + xl;
    const bool col_ok = x < A.W;
    float cx[4] = {0.f, 0.f, 0.f, 0.f};
    int cl[4] = {0, 0, 0, 0};
    if (col_ok) {
        int sx;
        float tx;
        cubic_src(x, A.sx, sx, tx);
        cubic_coeffs_f32(tx, cx);
#pragma unroll
        for (int j = 0; j < 4; ++j) cl[j] = cubic_clamp(cubic_clamp(sx - 1 + j, A.cw) - col_lo, CB_FOOT_W);
    }

    // vertical pass: rows y0 + 8 wv + i, i < 8, of this thread's column; the four footprint rows of each packed into one register
    const int ya = y0 + wv * CB_ROWS_PER_THREAD;
    const int n_ok = col_ok ? min(max(A.H - ya, 0), CB_ROWS_PER_THREAD) : 0;
    float cy[CB_ROWS_PER_THREAD][4];
    unsigned rl[CB_ROWS_PER_THREAD];
#pragma unroll
    for (int i = 0; i < CB_ROWS_PER_THREAD; ++i) {
        rl[i] = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) cy[i][j] = 0.f;
        if (i < n_ok) {
            int sy;
            float ty;
            cubic_src(ya + i, A.sy, sy, ty);
            cubic_coeffs_f32(ty, cy[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) rl[i] |= (unsigned)cubic_clamp(cubic_clamp(sy - 1 + j, A.ch) - row_lo, CB_FOOT_H) << (8 * j);
        }
    }

    const size_t plane = (size_t)A.h * A.w;
    const size_t HW = (size_t)A.H * A.W;
    const size_t out0 = (size_t)ya * A.W + x;            // this thread's first pixel within an output plane
    float best[CB_ROWS_PER_THREAD];
    int best_k[CB_ROWS_PER_THREAD];
#pragma unroll
    for (int i = 0; i < CB_ROWS_PER_THREAD; ++i) { best[i] = 0.f; best_k[i] = 0; }

    for (int k = 0; k < A.K; ++k) {
        const float* pa = A.a + ((size_t)b * A.K + k) * plane;
        const float* pb = A.b ? A.b + ((size_t)b * A.K + (A.permuted ? A.perm.get(k) : k)) * plane : nullptr;
#pragma unroll
        for (int q = 0; q < CB_STAGE; ++q)
            if (st_off[q] >= 0) stage[st_lds[q]] = cubic_value(pa, pb, st_off[q], st_offm[q]);
        __syncthreads();          // the footprint is staged; the vertical pass of class k - 1 is behind every thread
        if (col_ok) {
#pragma unroll
            for (int q = 0; q < CB_HZ_ROWS; ++q) {
                const int r = wv + 4 * q;
                if (r < nrows) {
                    const float* s = stage + r * CB_FOOT_W;
                    hzb[r * CB_TILE_W + xl] = cubic_dot(s[cl[0]], s[cl[1]], s[cl[2]], s[cl[3]], cx);
                }
            }
        }
        __syncthreads();          // the horizontal pass is complete; stage may be overwritten
        float* fk = fused ? fused + ((size_t)b * A.K + k) * HW + out0 : nullptr;
#pragma unroll
        for (int i = 0; i < CB_ROWS_PER_THREAD; ++i) {
            if (i < n_ok) {
                const unsigned r = rl[i];
                const float v = cubic_dot(hzb[(r & 255u) * CB_TILE_W + xl], hzb[((r >> 8) & 255u) * CB_TILE_W + xl],
                                          hzb[((r >> 16) & 255u) * CB_TILE_W + xl], hzb[(r >> 24) * CB_TILE_W + xl], cy[i]);
                if (fk) fk[(size_t)i * A.W] = v;
                if (k == 0 || v > best[i]) { best[i] = v; best_k[i] = k; }
            }
        }
    }
    if (pred) {
#pragma unroll
        for (int i = 0; i < CB_ROWS_PER_THREAD; ++i)
            if (i < n_ok) pred[(size_t)b * HW + out0 + (size_t)i * A.W] = (uint8_t)best_k[i];
    }
}

// path 0, where both paths are legal: the tiled one when its grid fills the device, else the direct one. Measured on the MI355X
// (profiles/val_cubic_timing.json): 8 x 19 x 256 x 512 -> 1024 x 2048, 8192 tiles: tiled 0.311 ms, direct 0.874 ms;
// 1 x 171 x 130 x 130 -> 520 x 520, 153 tiles on 256 compute units, each walking 171 classes between barriers: tiled 0.224 ms,
// direct 0.219 ms.
constexpr long CB_MIN_TILES = 256;

}  // namespace

extern "C" int cseg_cubic_argmax(const float* a, const float* b, const uint8_t* perm, int B, int K, int h, int w, int ch, int cw,
                                 int H, int W, int path, uint8_t* pred, float* fused, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(K >= 1 && K <= MS_MAX_K, "cubic_argmax: K = %d classes (the prediction is one byte; 1 to %d)", K, MS_MAX_K);
    CSEG_REQUIRE(B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "cubic_argmax: empty shape (B = %d, h x w = %d x %d, H x W = %d x %d)", B, h,
                 w, H, W);
    CSEG_REQUIRE(a, "cubic_argmax: a is null");
    CSEG_REQUIRE(ch >= 1 && ch <= h && cw >= 1 && cw <= w, "cubic_argmax: the crop (ch, cw) = (%d, %d) is outside the %d x %d map", ch,
                 cw, h, w);
    CSEG_REQUIRE(!perm || b, "cubic_argmax: perm was given without b, the mirrored operand whose classes it permutes");
    CSEG_REQUIRE(pred || fused, "cubic_argmax: both outputs (pred, fused) are null");
    CSEG_REQUIRE(path >= 0 && path <= 2, "cubic_argmax: path = %d (0 = the library's choice, 1 = direct, 2 = tiled)", path);
    CSEG_REQUIRE((long)B * H * W < 2147483647L, "cubic_argmax: B x H x W = %d x %d x %d output pixels do not fit 31 bits", B, H, W);
    CSEG_REQUIRE((long)h * w < 2147483647L, "cubic_argmax: the map is too large (h x w = %d x %d)", h, w);
    const bool tiled_ok = (long)H >= 2L * ch && (long)W >= 2L * cw;
    CSEG_REQUIRE(path != 2 || tiled_ok, "cubic_argmax: path = 2 (tiled) covers upsampling by at least 2 in both axes, not a %d x %d crop "
                 "to %d x %d", ch, cw, H, W);
    CubicArgs A;
    A.a = a; A.b = b;
    A.B = B; A.K = K; A.h = h; A.w = w; A.ch = ch; A.cw = cw; A.H = H; A.W = W;
    A.sy = 1.0 / ((double)H / (double)ch);
    A.sx = 1.0 / ((double)W / (double)cw);
    A.permuted = perm ? 1 : 0;
    for (int j = 0; j < MS_MAX_K / 4; ++j) A.perm.w[j] = 0u;
    if (perm) {                          // everything is checked before the launch: a refused table launches nothing
        int at = 0, val = 0;
        const char* fault = ms_perm_fault(perm, K, &at, &val);
        CSEG_REQUIRE(!fault, "cubic_argmax: perm[%d] = %d %s (perm must be a permutation of the %d classes)", at, val, fault, K);
        A.perm.fill(perm, K);
    }
    const int tiles_y = (H + CB_TILE_H - 1) / CB_TILE_H, tiles_x = (W + CB_TILE_W - 1) / CB_TILE_W;
    if (path == 0) path = tiled_ok && (long)B * tiles_y * tiles_x >= CB_MIN_TILES ? 2 : 1;
    if (path == 2) {
        const unsigned blocks = (unsigned)((long)B * tiles_y * tiles_x);                 // <= B * H * W < 2^31
        hipLaunchKernelGGL(cubic_tiled_kernel, dim3(blocks), dim3(256), 0, stream, A, tiles_y, tiles_x, pred, fused);
        CSEG_CHECK_LAUNCH("cubic_tiled_kernel");
    } else {
        const unsigned blocks = (unsigned)(((long)B * H * W + 255) / 256);
        hipLaunchKernelGGL(cubic_direct_kernel, dim3(blocks), dim3(256), 0, stream, A, pred, fused);
        CSEG_CHECK_LAUNCH("cubic_direct_kernel");
    }
    return 1;
}
