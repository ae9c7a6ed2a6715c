// Segmentation term with online hard example mining: FSOhemCELoss of the reference (lib/loss/loss_helper.py:215-261) on the
// bilinear(align_corners=True) upsampling of the coarse logits, without the [B,K,H,W] tensor, without a sort and without a host round trip.
//   p_i   = softmax(logits_i)[target_i] at every valid pixel (label in [0, K)), n of them
//   k     = min(max(1, min_kept), n - 1);  kth = the element of 0-based rank k of p in ascending order
//   thr   = max(kth, fp32(thresh));  kept = {valid i : p_i < thr}  (strict: the rank-k pixel and its ties are not kept)
//   loss  = sum_kept w_t (lse - logit_t) / |kept|;  d loss / d logit = [kept] w_t (softmax - onehot) / |kept|
// p is defined ONCE, by ohem_prob_kernel, and stored: the selection, the reduction and the backward compare the stored bits with the
// stored threshold, so they agree on the kept set whatever rounding produced p. p >= 0, so the unsigned order of its bit pattern is its
// numeric order and the rank-k element is found by a most-significant-digit radix select over the 32 bits in three levels of
// 12 (of which [0, 1] uses the values 0 .. 0x3F8) / 10 / 10 bits, 1024 bins each.
// Launches (no block waits for another one; integer atomics only, so every count is exact and nothing depends on arrival order):
//   ohem_zero_kernel    the three histograms and the state words <- 0 (a kernel, not hipMemsetAsync: DESIGN.md section 20.6)
//   ohem_prob_kernel    the cell softmax of ce_fwd_kernel (CeCell) -> p, nll = lse - v_t, lse per label pixel (p = 2 at
//                       invalid pixels), the level-0 histogram (block-private LDS bins, one lane merges the equal bins of its cell before
//                       the LDS atomic, non-empty bins flushed with global atomics) and #{p < thresh}
//   ohem_pick_kernel    one block, one thread per bin: prefix sum of a level's histogram -> the bin that holds rank k and the rank inside
//                       it. Level 0 also fixes n and k and takes the shortcut: #{p < thresh} >= k + 1 means kth < thresh, thr = thresh and
//                       levels 1 and 2 return at once. Level 2 completes the 32 bits of kth and writes thr.
//   ohem_hist_kernel    levels 1 and 2: histogram of the next digit of the stored p that match the prefix found so far (level 0 too when
//                       the caller has p but no level-0 histogram: the stage function of the tests)
//   ohem_reduce_kernel  fixed-order block partials (float64 sum of w_t nll, count) over p < thr;  ohem_finish_kernel  -> out, outi
//   ce_bwd_kernel<.., OHEM = true>  the backward of upsample_ce.hip with the coefficient above (cseg_upsample_ce.h)
// Algorithmic bytes at 8 x 19 x 128 x 256 -> 512 x 1024: forward seg 19.9 MB + target 33.6 MB read, p / nll / lse 3 x 16.8 MB written,
// p read 2 - 3 times by the select (16.8 MB each, L2 / MALL resident), p + nll (+ target with class weights) by the reduction; backward as
// the CE backward + p.
#include "cseg_upsample_ce.h"

namespace {

constexpr int OH_BINS = 1024;
constexpr int OH_STATE = 3 * OH_BINS;       // sel = [hist level 0 | hist level 1 | hist level 2 | state]
constexpr int OH_SEL_INTS = OH_STATE + 16;
constexpr float OH_SENTINEL = 2.0f;         // p of an invalid pixel: above every probability, never selected, never kept
enum { ST_BELOW = 0, ST_N, ST_K, ST_PREFIX, ST_RANK, ST_DONE, ST_KTH, ST_THR };

__device__ __forceinline__ unsigned oh_key(float p) { return __builtin_bit_cast(unsigned, p); }
__device__ __forceinline__ int oh_bin0(float p) { return (int)min(oh_key(p) >> 20, (unsigned)(OH_BINS - 1)); }

__global__ __launch_bounds__(256) void ohem_zero_kernel(int32_t* __restrict__ sel) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < OH_SEL_INTS) sel[i] = 0;
}

// the block's LDS bins -> the global histogram; the block's #{p < thresh} -> the state word (level 0 only)
__device__ __forceinline__ void oh_flush(const int* s_hist, int* s_red, int below, bool count_below, int32_t* __restrict__ hist,
                                         int32_t* __restrict__ state) {
    if (count_below) {
        below = wave_sum_i(below);
        if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = below;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < OH_BINS; i += 256)
        if (s_hist[i]) atomicAdd(&hist[i], s_hist[i]);
    if (count_below && threadIdx.x == 0) {
        const int total = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        if (total) atomicAdd(&state[ST_BELOW], total);
    }
}

template <int PX>
__global__ __launch_bounds__(256) void ohem_prob_kernel(const float* __restrict__ seg, const int64_t* __restrict__ target, CeDims d,
                                                        float thresh, float* __restrict__ p_out, float* __restrict__ nll_out,
                                                        float* __restrict__ lse_out, int32_t* __restrict__ sel,
                                                        int32_t* __restrict__ status) {
    __shared__ int s_hist[OH_BINS];
    __shared__ int s_red[4];
    for (int i = threadIdx.x; i < OH_BINS; i += 256) s_hist[i] = 0;
    __syncthreads();
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    int below = 0;
    CeCell<PX, true> cell;
    if (g < (long)d.B * d.H * d.w && cell.softmax(seg, target, d, g, status)) {
        const size_t o0 = cell.o0;
        int cur = -1, cnt = 0;                                    // run of equal bins inside the cell: one LDS atomic per run
#pragma unroll
        for (int p = 0; p < PX; ++p) {
            if (p < cell.n) {
                const float lse = cell.lse(p);
                float pv = OH_SENTINEL, nl = 0.f;
                if (cell.t[p] >= 0) {
                    pv = cell.et[p] / cell.se[p];                 // et is one of the non-negative terms of se: 0 <= p <= 1
                    nl = lse - cell.vt[p];                        // not -log p: stays finite where p underflows to 0
                }
                p_out[o0 + p] = pv;
                nll_out[o0 + p] = nl;
                if (lse_out) lse_out[o0 + p] = lse;
                if (pv <= 1.0f) {
                    below += pv < thresh ? 1 : 0;
                    const int bin = oh_bin0(pv);
                    if (bin != cur) {
                        if (cnt) atomicAdd(&s_hist[cur], cnt);
                        cur = bin; cnt = 0;
                    }
                    ++cnt;
                }
            }
        }
        if (cnt) atomicAdd(&s_hist[cur], cnt);
    }
    oh_flush(s_hist, s_red, below, true, sel, sel + OH_STATE);
}

// level 0: every valid p, digit = bits 31..20 (+ #{p < thresh}); level 1: p whose bits 31..20 equal the prefix, digit = bits 19..10;
// level 2: p whose bits 31..10 equal the prefix, digit = bits 9..0. A grid-stride loop over a fixed grid.
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ p, long P, int level, float thresh,
                                                        int32_t* __restrict__ sel) {
    __shared__ int s_hist[OH_BINS];
    __shared__ int s_red[4];
    const int32_t* state = sel + OH_STATE;
    if (level > 0 && state[ST_DONE]) return;                      // block-uniform: the shortcut was taken
    const unsigned prefix = level > 0 ? (unsigned)state[ST_PREFIX] : 0u;
    for (int i = threadIdx.x; i < OH_BINS; i += 256) s_hist[i] = 0;
    __syncthreads();
    int below = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        const float v = p[i];
        if (!(v <= 1.0f)) continue;                               // the sentinel of an invalid pixel
        const unsigned key = oh_key(v);
        unsigned digit;
        bool match = true;
        if (level == 0) { digit = key >> 20; below += v < thresh ? 1 : 0; }
        else if (level == 1) { digit = (key >> 10) & 1023u; match = (key >> 20) == prefix; }
        else { digit = key & 1023u; match = (key >> 10) == prefix; }
        if (match) atomicAdd(&s_hist[min(digit, (unsigned)(OH_BINS - 1))], 1);
    }
    oh_flush(s_hist, s_red, below, level == 0, sel + level * OH_BINS, sel + OH_STATE);
}

__global__ __launch_bounds__(1024) void ohem_pick_kernel(int level, float thresh, int min_kept, int shortcut, int32_t* __restrict__ sel) {
    __shared__ int s_wave[16];
    __shared__ int s_found[2];
    int32_t* state = sel + OH_STATE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (level > 0 && state[ST_DONE]) return;                      // (read by every thread before the first barrier, written after the last)
    int rank = level > 0 ? state[ST_RANK] : 0;
    const unsigned prefix = level > 0 ? (unsigned)state[ST_PREFIX] : 0u;
    const int below = state[ST_BELOW];
    if (tid == 0) { s_found[0] = 0; s_found[1] = 0; }
    const int cnt = sel[level * OH_BINS + tid];
    const int incl = wave_incl_scan_i(cnt, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int base = 0, total = 0;
    for (int i = 0; i < 16; ++i) {
        if (i < wave) base += s_wave[i];
        total += s_wave[i];
    }
    const int excl = base + incl - cnt;
    int k = 0;
    if (level == 0) {
        k = min(max(1, min_kept), total - 1);
        if (k < 0) k = 0;
        rank = k;
    }
    if (cnt > 0 && rank >= excl && rank < excl + cnt) { s_found[0] = tid; s_found[1] = rank - excl; }      // at most one thread
    __syncthreads();
    if (tid == 0) {
        const unsigned digit = (unsigned)s_found[0];              // a thread index: below OH_BINS by construction
        state[ST_RANK] = s_found[1];
        if (level == 0) {
            state[ST_N] = total;
            state[ST_K] = k;
            state[ST_PREFIX] = (int)digit;
            const int done = total == 0 || (shortcut && below >= k + 1);
            state[ST_DONE] = done;
            state[ST_KTH] = 0;
            state[ST_THR] = (int)oh_key(thresh);                  // what levels 1 and 2 overwrite unless the shortcut holds
        } else if (level == 1) {
            state[ST_PREFIX] = (int)((prefix << 10) | digit);
        } else {
            const unsigned key = (prefix << 10) | digit;
            state[ST_KTH] = (int)key;
            state[ST_THR] = (int)oh_key(fmaxf(__builtin_bit_cast(float, key), thresh));
        }
    }
}

__global__ __launch_bounds__(256) void ohem_reduce_kernel(const float* __restrict__ p, const float* __restrict__ nll,
                                                          const int64_t* __restrict__ target, const float* __restrict__ weight, int K,
                                                          long P, const int32_t* __restrict__ sel, double* __restrict__ partial,
                                                          int32_t* __restrict__ pcount) {
    __shared__ double s_sum[4];
    __shared__ int s_cnt[4];
    const float thr = __builtin_bit_cast(float, (unsigned)sel[OH_STATE + ST_THR]);
    double acc = 0.0;
    int cnt = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long)gridDim.x * 256) {
        const float v = p[i];
        if (v <= 1.0f && v < thr) {
            float wt = 1.f;
            if (weight) {
                const int64_t t64 = target[i];
                wt = weight[t64 < 0 ? 0 : (t64 >= K ? K - 1 : (int)t64)];      // (a kept pixel has a label in [0, K))
            }
            acc += (double)(wt * nll[i]);
            ++cnt;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    cnt = wave_sum_i(cnt);
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = acc; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        pcount[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    }
}

__global__ __launch_bounds__(1024) void ohem_finish_kernel(const double* __restrict__ partial, const int32_t* __restrict__ pcount,
                                                           int n_blocks, const int32_t* __restrict__ sel, float* __restrict__ out,
                                                           int32_t* __restrict__ outi) {
    __shared__ double red[2][16];
    double a = 0.0, c = 0.0;                                      // counts below 2^31 are exact in float64
    for (int i = threadIdx.x; i < n_blocks; i += 1024) { a += partial[i]; c += (double)pcount[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); c += __shfl_xor(c, o, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sc = 0.0;
        for (int i = 0; i < 16; ++i) { sa += red[0][i]; sc += red[1][i]; }
        const int32_t* state = sel + OH_STATE;
        out[0] = sc > 0.0 ? (float)(sa / sc) : __builtin_nanf("");      // nothing kept: the reference's mean of an empty tensor
        out[1] = (float)sc;
        out[2] = __builtin_bit_cast(float, (unsigned)state[ST_THR]);
        out[3] = (float)state[ST_N];
        outi[0] = (int32_t)sc;
        outi[1] = state[ST_N];
        outi[2] = state[ST_K];
        outi[3] = state[ST_DONE];
    }
}

int oh_grid(long P) {
    const long nb = (P + 2047) / 2048;
    return (int)(nb < 1 ? 1 : (nb > 1024 ? 1024 : nb));
}

}  // namespace

extern "C" int cseg_ohem_sel_ints(void) { return OH_SEL_INTS; }

extern "C" int cseg_ohem_reduce_blocks(long P) { return oh_grid(P); }

extern "C" int cseg_ohem_prob(const float* seg, const int64_t* target, int ignore_label, int B, int K, int h, int w, int H, int W,
                              float thresh, float* p, float* nll, float* lse, int32_t* sel, int32_t* status, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CeDims d;
    if (!make_dims(&d, B, K, h, w, H, W, ignore_label)) return 0;
    CSEG_REQUIRE((long)B * H * W < 2147483647L, "ohem_prob: %ld label pixels (B * H * W must be below 2^31)", (long)B * H * W);
    const int px = pick_px(max_cell_px(d));
    CSEG_REQUIRE(px > 0, "ohem_prob: %d label pixels share one coarse tap (%d -> %d); at most %d are supported", max_cell_px(d), w, W, MAX_PX);
    CSEG_REQUIRE(p && nll && sel, "ohem_prob: p, nll and sel are required");
    hipLaunchKernelGGL(ohem_zero_kernel, dim3((OH_SEL_INTS + 255) / 256), dim3(256), 0, stream, sel);
    CSEG_CHECK_LAUNCH("ohem_zero_kernel");
    const long n_cells = (long)B * H * w;
    const int n_blocks = (int)((n_cells + 255) / 256);
#define LAUNCH(P) hipLaunchKernelGGL(ohem_prob_kernel<P>, dim3(n_blocks), dim3(256), 0, stream, seg, target, d, thresh, p, nll, lse, sel, status)
    CE_BY_PX(px, LAUNCH);
#undef LAUNCH
    CSEG_CHECK_LAUNCH("ohem_prob_kernel");
    return 1;
}

extern "C" int cseg_ohem_select(const float* p, long P, float thresh, int min_kept, int shortcut, int have_level0, int32_t* sel,
                                cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(p && sel, "ohem_select: p and sel are required");
    CSEG_REQUIRE(P >= 1 && P < 2147483647L, "ohem_select: %ld pixels (1 <= P < 2^31)", P);
    CSEG_REQUIRE(thresh == thresh, "ohem_select: the threshold is NaN");
    const int grid = oh_grid(P);
    if (!have_level0) {
        hipLaunchKernelGGL(ohem_zero_kernel, dim3((OH_SEL_INTS + 255) / 256), dim3(256), 0, stream, sel);
        CSEG_CHECK_LAUNCH("ohem_zero_kernel");
        hipLaunchKernelGGL(ohem_hist_kernel, dim3(grid), dim3(256), 0, stream, p, P, 0, thresh, sel);
        CSEG_CHECK_LAUNCH("ohem_hist_kernel");
    }
    for (int level = 0; level < 3; ++level) {
        if (level > 0) {
            hipLaunchKernelGGL(ohem_hist_kernel, dim3(grid), dim3(256), 0, stream, p, P, level, thresh, sel);
            CSEG_CHECK_LAUNCH("ohem_hist_kernel");
        }
        hipLaunchKernelGGL(ohem_pick_kernel, dim3(1), dim3(1024), 0, stream, level, thresh, min_kept, shortcut, sel);
        CSEG_CHECK_LAUNCH("ohem_pick_kernel");
    }
    return 1;
}

extern "C" int cseg_ohem_reduce(const float* p, const float* nll, const int64_t* target, const float* weight, int K, long P,
                                const int32_t* sel, double* partial, int32_t* pcount, float* out, int32_t* outi, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(p && nll && sel && partial && pcount && out && outi, "ohem_reduce: a required buffer is missing");
    CSEG_REQUIRE(!weight || target, "ohem_reduce: class weights need the labels");
    CSEG_REQUIRE(K >= 1 && P >= 1 && P < 2147483647L, "ohem_reduce: K = %d, P = %ld (K >= 1, 1 <= P < 2^31)", K, P);
    const int grid = oh_grid(P);
    hipLaunchKernelGGL(ohem_reduce_kernel, dim3(grid), dim3(256), 0, stream, p, nll, target, weight, K, P, sel, partial, pcount);
    CSEG_CHECK_LAUNCH("ohem_reduce_kernel");
    hipLaunchKernelGGL(ohem_finish_kernel, dim3(1), dim3(1024), 0, stream, partial, pcount, grid, sel, out, outi);
    CSEG_CHECK_LAUNCH("ohem_finish_kernel");
    return 1;
}

extern "C" int cseg_ohem_bwd(const float* seg, const int64_t* target, const float* weight, int ignore_label, int B, int K, int h, int w,
                             int H, int W, const float* p, const float* lse, const float* out, const int32_t* outi, const float* d_loss,
                             float* d_seg, cseg_stream_t stream_) {
    CSEG_REQUIRE(p && out && outi, "ohem_bwd: needs p, out and outi of the forward");
    return launch_ce_bwd<true>("ohem_bwd", seg, target, weight, ignore_label, B, K, h, w, H, W, out, d_loss, lse, d_seg, p, outi,
                               (hipStream_t)stream_);
}
