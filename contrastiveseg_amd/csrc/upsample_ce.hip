// Segmentation term: bilinear(align_corners=True) upsample of the logits to label resolution fused with the
// weighted cross entropy (ignore index, mean over the sum of weights).
// Reference: lib/loss/loss_contrast.py:180-181 + lib/loss/loss_helper.py:169-206. The reference materialises the
// [B,K,H,W] logits (319 MB at bs8) and makes ~3 passes over them forward plus the same again backward; here the
// upsampled tensor never exists.
//
// Work decomposition (round 2; replaces the LDS-tile kernels whose backward ran a serial loop over the K classes with
// three barriers each): a CELL = the fine pixels of one label row that share the left coarse tap x0 = c (4-5 pixels at
// the 4.02x upsampling of the HRNet head, 1 at label resolution, <= 17). One lane owns one coarse column c, so the
// four coarse logits a cell needs per class are loaded with unit stride across the wave straight from L1/L2 -- no LDS
// tile, no bank conflicts -- the vertical blend is done once per class and every fine pixel costs two FMAs.
//   forward   one thread per (label row, cell): max pass + sum-exp pass over the classes, log-sum-exp written to a
//             [B,H,W] buffer for the backward, fixed-order block partials of (weighted nll, weight).
//   backward  a block = (image, band of R coarse rows, group of KG classes); lane = coarse column. The block marches
//             down the label rows of its band; per row each lane evaluates g_k = coef * (softmax_k - onehot_k) for
//             its cell, splits it into the part that lands on column c and the part for column c+1 (handed to the
//             right neighbour with one DPP shift; one LDS word per wave boundary), and accumulates the two coarse rows
//             the label row touches in registers (a sliding pair: the march is monotone). Every exp is evaluated once
//             per (pixel, class), all lanes work on all classes of the group, no atomics: run-to-run deterministic.
// HBM-bound (algorithmic bytes: seg + target [+ lse] forward; seg + target + lse + d_seg backward); no MFMA.
#include "cseg_upsample_ce.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------
template <int PX>
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ seg, const int64_t* __restrict__ target,
                                                     const float* __restrict__ weight, CeDims d, float* __restrict__ lse_out,
                                                     float* __restrict__ partial, int32_t* __restrict__ status) {
    __shared__ float red[2][4];
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long n_cells = (long)d.B * d.H * d.w;
    float wnll = 0.f, wsum = 0.f;
    if (g < n_cells) {
        const int c = (int)(g % d.w);
        const long row = g / d.w;
        const int Y = (int)(row % d.H), b = (int)(row / d.H);
        const int Xs = first_with_tap(d.sx, d.W, c), Xe = first_with_tap(d.sx, d.W, c + 1);
        const int n = min(Xe - Xs, PX);
        if (n > 0) {
            int y0, y1;
            float ly1;
            tap(d.sy, d.h, Y, y0, y1, ly1);
            const float ly0 = 1.f - ly1;
            const int c1 = c + (c < d.w - 1 ? 1 : 0);
            float lx1[PX], m[PX], se[PX], vt[PX];
            int t[PX];
            const int64_t* trow = target + ((size_t)b * d.H + Y) * d.W + Xs;
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                lx1[p] = 0.f; m[p] = -INFINITY; se[p] = 0.f; vt[p] = 0.f; t[p] = -1;
                if (p < n) {
                    lx1[p] = d.sx * (float)(Xs + p) - (float)c;
                    const int64_t t64 = trow[p];
                    if (t64 != (int64_t)d.ignore_label) {
                        if (t64 < 0 || t64 >= d.K) atomicAdd(&status[1], 1);
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
            for (int k = 0; k < d.K; ++k) {                       // pass 2: sum of exponentials, target logit
                const float r0 = ly0 * s0[k * plane + c] + ly1 * s1[k * plane + c];
                const float r1 = ly0 * s0[k * plane + c1] + ly1 * s1[k * plane + c1];
#pragma unroll
                for (int p = 0; p < PX; ++p) {
                    const float v = fmaf(lx1[p], r1 - r0, r0);
                    se[p] += __expf(v - m[p]);
                    vt[p] = (k == t[p]) ? v : vt[p];
                }
            }
            float* lrow = lse_out ? lse_out + ((size_t)b * d.H + Y) * d.W + Xs : nullptr;
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                if (p < n) {
                    const float lse = m[p] + __logf(se[p]);
                    if (lrow) lrow[p] = lse;
                    if (t[p] >= 0) {
                        const float wt = weight ? weight[t[p]] : 1.f;
                        wnll += wt * (lse - vt[p]);
                        wsum += wt;
                    }
                }
            }
        }
    }
    wnll = wave_sum(wnll);
    wsum = wave_sum(wsum);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = wnll; red[1][threadIdx.x >> 6] = wsum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x + 0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        partial[2 * (size_t)blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

__global__ __launch_bounds__(1024) void ce_finish_kernel(const float* __restrict__ partial, int n_blocks,
                                                         float* __restrict__ out) {
    __shared__ double red[2][16];
    double a = 0.0, w = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += 1024) { a += partial[2 * (size_t)i]; w += partial[2 * (size_t)i + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); w += __shfl_xor(w, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = w; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sw = 0.0;
        for (int i = 0; i < 16; ++i) { sa += red[0][i]; sw += red[1][i]; }
        out[0] = (float)(sa / sw);
        out[1] = (float)sw;
    }
}

}  // namespace

extern "C" int cseg_upsample_ce_blocks(int B, int H, int W) {
    // upper bound of the forward grid for any coarse width w <= W (one thread per (label row, coarse column))
    return (int)(((long)B * H * W + 255) / 256);
}

extern "C" int cseg_upsample_ce_fwd(const float* seg, const int64_t* target, const float* weight, int ignore_label,
                                    int B, int K, int h, int w, int H, int W, float* partial, float* out,
                                    int32_t* status, float* lse, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CeDims d;
    if (!make_dims(&d, B, K, h, w, H, W, ignore_label)) return 0;
    const int px = pick_px(max_cell_px(d));
    CSEG_REQUIRE(px > 0, "upsample_ce: %d label pixels share one coarse tap (%d -> %d); at most %d are supported", max_cell_px(d), w, W, MAX_PX);
    const long n_cells = (long)B * H * w;
    const int n_blocks = (int)((n_cells + 255) / 256);
#define LAUNCH(P) hipLaunchKernelGGL(ce_fwd_kernel<P>, dim3(n_blocks), dim3(256), 0, stream, seg, target, weight, d, lse, \
                                     partial, status)
    switch (px) {
        case 1: LAUNCH(1); break;
        case 2: LAUNCH(2); break;
        case 3: LAUNCH(3); break;
        case 5: LAUNCH(5); break;
        case 9: LAUNCH(9); break;
        default: LAUNCH(17); break;
    }
#undef LAUNCH
    CSEG_CHECK_LAUNCH("ce_fwd_kernel");
    hipLaunchKernelGGL(ce_finish_kernel, dim3(1), dim3(1024), 0, stream, partial, n_blocks, out);
    CSEG_CHECK_LAUNCH("ce_finish_kernel");
    return 1;
}

extern "C" int cseg_upsample_ce_bwd(const float* seg, const int64_t* target, const float* weight, int ignore_label,
                                    int B, int K, int h, int w, int H, int W, const float* out, const float* d_loss,
                                    const float* lse, float* d_seg, cseg_stream_t stream_) {
    return launch_ce_bwd<false>("upsample_ce_bwd", seg, target, weight, ignore_label, B, K, h, w, H, W, out, d_loss, lse, d_seg, nullptr, nullptr,
                                (hipStream_t)stream_);
}
