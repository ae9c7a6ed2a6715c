// Shared between upsample_ce.hip (weighted CE, mean over the sum of weights) and ohem.hip (CE over the mined pixels, mean over their
// count): the cell softmax of the forward (one lane per label row and cell) and the backward kernel, which
// differs between the two only in the per-pixel coefficient (template flag OHEM). Internal linkage on purpose: each of the two
// translation units instantiates its own kernels.
#pragma once
#include "cseg_taps.h"

namespace {

constexpr int BAND = 4;        // coarse rows per backward block
constexpr int MAX_PX = 17;     // fine pixels per cell (upsampling factors up to 16x)

struct CeDims : UpDims {
    int ignore_label;
};

// one case per cell size the kernels are instantiated for (pick_px)
#define CE_BY_PX(px, LAUNCH)           \
    switch (px) {                      \
        case 1: LAUNCH(1); break;      \
        case 2: LAUNCH(2); break;      \
        case 3: LAUNCH(3); break;      \
        case 5: LAUNCH(5); break;      \
        case 9: LAUNCH(9); break;      \
        default: LAUNCH(17); break;    \
    }

// ---------------------------------------------------------------------------------------------------------
// forward: the softmax statistics of one cell, global cell index g = (b * H + Y) * w + c
// ---------------------------------------------------------------------------------------------------------
// After softmax(), for the n label pixels at o0 .. o0 + n - 1: t = the label (-1: ignored or out of range, the latter counted in
// status[1]), m + log(se) = the log-sum-exp, vt = the target logit, et = exp(vt - m) (WANT_ET only).
template <int PX, bool WANT_ET>
struct CeCell {
    int n, t[PX];
    size_t o0;
    float m[PX], se[PX], vt[PX], et[WANT_ET ? PX : 1];

    // false: the cell has no label pixel
    __device__ __forceinline__ bool softmax(const float* __restrict__ seg, const int64_t* __restrict__ target, const CeDims& d, long g,
                                            int32_t* __restrict__ status) {
        const int c = (int)(g % d.w);
        const long row = g / d.w;
        const int Y = (int)(row % d.H), b = (int)(row / d.H);
        const int Xs = first_with_tap(d.sx, d.W, c), Xe = first_with_tap(d.sx, d.W, c + 1);
        n = min(Xe - Xs, PX);
        if (n <= 0) return false;
        int y0, y1;
        float ly1;
        bl_tap(d.sy, d.h, Y, y0, y1, ly1);
        const float ly0 = 1.f - ly1;
        const int c1 = c + (c < d.w - 1 ? 1 : 0);
        float lx1[PX];
        o0 = ((size_t)b * d.H + Y) * d.W + Xs;
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            lx1[p] = 0.f; m[p] = -INFINITY; se[p] = 0.f; vt[p] = 0.f; t[p] = -1;
            if constexpr (WANT_ET) et[p] = 0.f;
            if (p < n) {
                lx1[p] = d.sx * (float)(Xs + p) - (float)c;
                const int64_t t64 = target[o0 + p];
                if (t64 != (int64_t)d.ignore_label) {
                    if (t64 < 0 || t64 >= d.K) { if (status) atomicAdd(&status[1], 1); }
                    else t[p] = (int)t64;
                }
            }
        }
        const float* s0 = seg + (((size_t)b * d.K) * d.h + y0) * d.w;
        const float* s1 = seg + (((size_t)b * d.K) * d.h + y1) * d.w;
        const size_t plane = (size_t)d.h * d.w;
        for (int k = 0; k < d.K; ++k) {                       // pass 1: running max
            const float r0 = ly0 * s0[k * plane + c] + ly1 * s1[k * plane + c];
            const float r1 = ly0 * s0[k * plane + c1] + ly1 * s1[k * plane + c1];
#pragma unroll
            for (int p = 0; p < PX; ++p) m[p] = fmaxf(m[p], fmaf(lx1[p], r1 - r0, r0));
        }
        for (int k = 0; k < d.K; ++k) {                       // pass 2: sum of exponentials, target logit (and its exponential)
            const float r0 = ly0 * s0[k * plane + c] + ly1 * s1[k * plane + c];
            const float r1 = ly0 * s0[k * plane + c1] + ly1 * s1[k * plane + c1];
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const float v = fmaf(lx1[p], r1 - r0, r0);
                const float ev = __expf(v - m[p]);
                se[p] += ev;
                vt[p] = (k == t[p]) ? v : vt[p];
                if constexpr (WANT_ET) et[p] = (k == t[p]) ? ev : et[p];
            }
        }
        return true;
    }
    __device__ __forceinline__ float lse(int p) const { return m[p] + __logf(se[p]); }
};

// ---------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------
// OHEM (ohem.hip): a pixel takes part only when its stored probability lies below the mined threshold, and the mean is over the kept
// count: coefficient w_t * [prob < out[2]] * d_loss / outi[0] (0 when nothing was kept). `prob` and `outi` are not read otherwise.
template <int PX, int KG, bool OHEM>
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ seg, const int64_t* __restrict__ target,
                                                     const float* __restrict__ weight, const float* __restrict__ lse,
                                                     CeDims d, int n_groups, int n_bands, int halo,
                                                     const float* __restrict__ out, const float* __restrict__ d_loss,
                                                     float* __restrict__ d_seg, const float* __restrict__ prob,
                                                     const int32_t* __restrict__ outi) {
    __shared__ float xchg[2][4][KG];          // [row parity][wave][class]: hB of the wave's last lane
    int blk = blockIdx.x;
    const int grp = blk % n_groups; blk /= n_groups;
    const int band = blk % n_bands; blk /= n_bands;
    const int n_cb = (d.w + (256 - halo) - 1) / (256 - halo);
    const int cb = blk % n_cb;
    const int b = blk / n_cb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = cb * (256 - halo) + tid - halo;                 // this lane's cell / output column
    const bool cell_ok = c >= 0 && c < d.w;
    const bool writes = cell_ok && tid >= halo;                   // halo lane only feeds its right neighbour
    const int k0 = grp * KG;
    const int ys0 = band * BAND;
    const int ys_end = min(ys0 + BAND, d.h);                      // rows [ys0, ys_end) are written by this block
    const float gscale = OHEM ? (outi[0] > 0 ? d_loss[0] / (float)outi[0] : 0.f) : d_loss[0] / out[1];
    const float thr = OHEM ? out[2] : 0.f;

    const int Xs = cell_ok ? first_with_tap(d.sx, d.W, c) : 0;
    const int n = cell_ok ? min(first_with_tap(d.sx, d.W, c + 1) - Xs, PX) : 0;
    const int c1 = c + (c < d.w - 1 ? 1 : 0);
    float lx1[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) lx1[p] = p < n ? d.sx * (float)(Xs + p) - (float)c : 0.f;

    // label rows whose upper tap lies in [ys0 - 1, ys_end - 1]
    const int Y_lo = first_with_tap(d.sy, d.H, ys0 - 1), Y_hi = first_with_tap(d.sy, d.H, ys_end);
    float acc_lo[KG], acc_hi[KG];            // coarse rows y_cur and y_cur + 1
#pragma unroll
    for (int j = 0; j < KG; ++j) { acc_lo[j] = 0.f; acc_hi[j] = 0.f; }
    int y_cur = max(ys0 - 1, 0);
    if (Y_lo < Y_hi) y_cur = tap0(d.sy, Y_lo);

    auto flush_lo = [&](int row) {
        if (writes && row >= ys0 && row < ys_end) {
#pragma unroll
            for (int j = 0; j < KG; ++j)
                if (k0 + j < d.K) d_seg[(((size_t)b * d.K + k0 + j) * d.h + row) * d.w + c] = acc_lo[j];
        }
    };

    for (int Y = Y_lo; Y < Y_hi; ++Y) {
        int y0, y1;
        float ly1;
        bl_tap(d.sy, d.h, Y, y0, y1, ly1);
        const float ly0 = 1.f - ly1;
        while (y_cur < y0) {                 // the march is monotone: retire the finished coarse row
            flush_lo(y_cur);
#pragma unroll
            for (int j = 0; j < KG; ++j) { acc_lo[j] = acc_hi[j]; acc_hi[j] = 0.f; }
            ++y_cur;
        }
        float coef[PX], ls[PX];
        int t[PX];
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            coef[p] = 0.f; ls[p] = INFINITY; t[p] = -1;      // exp(v - inf) = 0: inactive pixels contribute exactly 0
            if (p < n) {
                const size_t o = ((size_t)b * d.H + Y) * d.W + Xs + p;
                const int64_t t64 = target[o];
                bool on = t64 != (int64_t)d.ignore_label && t64 >= 0 && t64 < d.K;
                if constexpr (OHEM) on = on && prob[o] < thr;
                if (on) {
                    t[p] = (int)t64;
                    coef[p] = (weight ? weight[t[p]] : 1.f) * gscale;
                    ls[p] = lse[o];
                }
            }
        }
        float hA[KG], hB[KG];
#pragma unroll
        for (int j = 0; j < KG; ++j) {
            hA[j] = 0.f; hB[j] = 0.f;
            const int k = k0 + j;
            if (k < d.K && n > 0) {
                const float* s0 = seg + (((size_t)b * d.K + k) * d.h + y0) * d.w;
                const float* s1 = seg + (((size_t)b * d.K + k) * d.h + y1) * d.w;
                const float r0 = ly0 * s0[c] + ly1 * s1[c];
                const float r1 = ly0 * s0[c1] + ly1 * s1[c1];
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    const float v = fmaf(lx1[p], r1 - r0, r0);
                    const float gk = coef[p] * (__expf(v - ls[p]) - (t[p] == k ? 1.f : 0.f));   // coef = 0: nothing
                    const float gb = lx1[p] * gk;
                    hB[j] += gb;                   // lands on column c + 1 (x1 tap)
                    hA[j] += gk - gb;              // lands on column c     (x0 tap, weight 1 - lx1)
                }
            }
        }
        // at the right image edge x1 == x0: both taps land on column c
        if (cell_ok && c == d.w - 1) {
#pragma unroll
            for (int j = 0; j < KG; ++j) { hA[j] += hB[j]; hB[j] = 0.f; }
        }
        const int par = Y & 1;
        if (lane == 63) {
#pragma unroll
            for (int j = 0; j < KG; ++j) xchg[par][wave][j] = hB[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KG; ++j) {
            float left = __shfl_up(hB[j], 1, 64);
            if (lane == 0) left = wave > 0 ? xchg[par][wave - 1][j] : 0.f;
            const float H = hA[j] + left;
            if (y1 == y0) acc_lo[j] += H;          // bottom edge: both vertical taps on the same coarse row
            else { acc_lo[j] += ly0 * H; acc_hi[j] += ly1 * H; }
        }
    }
    flush_lo(y_cur);
#pragma unroll
    for (int j = 0; j < KG; ++j) acc_lo[j] = acc_hi[j];
    flush_lo(y_cur + 1);
    // coarse rows of the band that no label row touches (cannot happen when upsampling; kept for safety)
    for (int row = max(y_cur + 2, ys0); row < ys_end; ++row) {
#pragma unroll
        for (int j = 0; j < KG; ++j) acc_lo[j] = 0.f;
        flush_lo(row);
    }
    if (Y_lo >= Y_hi) {
        for (int row = ys0; row < ys_end; ++row) {
#pragma unroll
            for (int j = 0; j < KG; ++j) acc_lo[j] = 0.f;
            flush_lo(row);
        }
    }
}

int make_dims(CeDims* d, int B, int K, int h, int w, int H, int W, int ignore_label) {
    d->ignore_label = ignore_label;
    return up_dims("upsample_ce", d, B, K, h, w, H, W);
}

// largest number of fine pixels that share one left tap (host side, exact: same float arithmetic as the device)
int max_cell_px(const CeDims& d) {
    int best = 0, run = 0, prev = -1;
    for (int X = 0; X < d.W; ++X) {
        const int x0 = tap0(d.sx, X);
        run = (x0 == prev) ? run + 1 : 1;
        prev = x0;
        if (run > best) best = run;
    }
    return best;
}

int pick_px(int need) {
    const int opts[] = {1, 2, 3, 5, 9, 17};
    for (int o : opts)
        if (need <= o) return o;
    return 0;
}

int pick_kg(int K) {
    const int opts[] = {8, 6, 5, 4};
    int best = 4, waste = 1 << 30;
    for (int o : opts) {
        const int wst = (K + o - 1) / o * o - K;
        if (wst < waste) { waste = wst; best = o; }
    }
    return best;
}

// the backward launch of both terms; `what` names the caller in the refusals
template <bool OHEM>
int launch_ce_bwd(const char* what, const float* seg, const int64_t* target, const float* weight, int ignore_label, int B, int K, int h,
                  int w, int H, int W, const float* out, const float* d_loss, const float* lse, float* d_seg, const float* prob,
                  const int32_t* outi, hipStream_t stream) {
    CeDims d;
    if (!make_dims(&d, B, K, h, w, H, W, ignore_label)) return 0;
    CSEG_REQUIRE(lse, "%s: needs the log-sum-exp buffer written by the forward", what);
    const int px = pick_px(max_cell_px(d));
    CSEG_REQUIRE(px > 0, "upsample_ce: %d label pixels share one coarse tap (%d -> %d); at most %d are supported", max_cell_px(d), w, W, MAX_PX);
    const int kg = pick_kg(K);
    const int n_groups = (K + kg - 1) / kg, n_bands = (h + BAND - 1) / BAND;
    const int halo = w > 256 ? 1 : 0;
    const int n_cb = (w + (256 - halo) - 1) / (256 - halo);
    const int threads = n_cb > 1 ? 256 : ((w + 63) / 64) * 64;
    const long n_blocks = (long)B * n_cb * n_bands * n_groups;
    CSEG_REQUIRE(n_blocks < 2147483647L, "%s: grid too large", what);
#define LAUNCH(P, G) hipLaunchKernelGGL((ce_bwd_kernel<P, G, OHEM>), dim3((unsigned)n_blocks), dim3(threads), 0, stream, seg, target, \
                                        weight, lse, d, n_groups, n_bands, halo, out, d_loss, d_seg, prob, outi)
#define BY_KG(P)                                   \
    switch (kg) {                                  \
        case 8: LAUNCH(P, 8); break;               \
        case 6: LAUNCH(P, 6); break;               \
        case 5: LAUNCH(P, 5); break;               \
        default: LAUNCH(P, 4); break;              \
    }
    CE_BY_PX(px, BY_KG);
#undef BY_KG
#undef LAUNCH
    CSEG_CHECK_LAUNCH("ce_bwd_kernel");
    return 1;
}

}  // namespace
