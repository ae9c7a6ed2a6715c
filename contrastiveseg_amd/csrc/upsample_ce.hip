// Segmentation term: bilinear(align_corners=True) upsample of the logits to label resolution fused with the
// weighted cross entropy (ignore index, mean over the sum of weights).
// Reference: lib/loss/loss_contrast.py:180-181 + lib/loss/loss_helper.py:169-206. The reference materialises the
// [B,K,H,W] logits (319 MB at bs8) and makes ~3 passes over them forward plus the same again backward; here the
// upsampled tensor never exists.
//
// Work decomposition: the cells of DESIGN.md section 26 (one lane owns one coarse column; cseg_upsample_ce.h).
//   forward   one thread per (label row, cell): max pass + sum-exp pass over the classes (CeCell), log-sum-exp written
//             to a [B,H,W] buffer for the backward, fixed-order block partials of (weighted nll, weight).
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
    float wnll = 0.f, wsum = 0.f;
    CeCell<PX, false> cell;
    if (g < (long)d.B * d.H * d.w && cell.softmax(seg, target, d, g, status)) {
        float* lrow = lse_out ? lse_out + cell.o0 : nullptr;
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            if (p < cell.n) {
                const float lse = cell.lse(p);
                if (lrow) lrow[p] = lse;
                if (cell.t[p] >= 0) {
                    const float wt = weight ? weight[cell.t[p]] : 1.f;
                    wnll += wt * (lse - cell.vt[p]);
                    wsum += wt;
                }
            }
        }
    }
    block_pair_to_partial(wave_sum(wnll), wave_sum(wsum), red, partial);
}

__global__ __launch_bounds__(1024) void ce_finish_kernel(const float* __restrict__ partial, int n_blocks,
                                                         float* __restrict__ out) {
    __shared__ double red[2][16];
    double a = 0.0, w = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += 1024) { a += partial[2 * (size_t)i]; w += partial[2 * (size_t)i + 1]; }
    a = wave_sum_d(a);
    w = wave_sum_d(w);
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
    CE_BY_PX(px, LAUNCH);
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
