// Test phase: multi-scale + flip fusion with the argmax, and the confusion matrix.
// Reference: segmentor/tester.py:310-327 (ss_test: forward at one scale, F.interpolate(bilinear, align_corners=True) back to the
// input size) and :380-398 (ms_test: per scale probs = U(a) + flip(U(b)), full_probs += weight * probs), followed by the argmax of
// :189; lib/metrics/running_score.py _fast_hist for the scoring. The reference makes about ten passes over a [B,K,H,W] tensor per
// scale (159 MB per image at Cityscapes size); upsampling, flipping and the weighted sum are linear, only the argmax is not, so
// here none of the full-resolution tensors exists: one kernel reads the coarse maps (1/16 of the pixels each at stride 4; L1/L2
// hits) and writes one byte per pixel.
//
// ms_fuse_kernel   lives in cseg_ms_fuse.h; this file launches its MsArgs instances, ms_eval_ragged.hip the RgArgs ones.
//                  One thread per output pixel. The taps of every term (row offsets, columns, blend factors; for the flipped map
//                  the taps of the MIRRORED output column W-1-x, which is what flipping the upsampled map means) are computed once
//                  with the package's fp32 index arithmetic (bl_tap) and stay in registers: the term loop is unrolled
//                  to the template's NT. Classes run in the outer loop, terms inside, in the reference's association order
//                      v = 0;  v = v + w_i * (U(a_i)[y,x] + U(b_i)[y,W-1-x])
//                  with a running (best, index) pair: no per-thread array over K. Strict '>' keeps the first index among equal
//                  maxima (torch.argmax / np.argmax). U blends vertically first, then one fused multiply-add across the columns;
//                  floating-point contraction is switched off in the kernel so that every other rounding is where the source
//                  puts it, on the GPU and on the emulated device alike. No atomics: deterministic.
//                  cseg_ms_fuse_argmax_perm: the flipped map's term becomes U(b_i)[perm[k]][y,W-1-x] -- the classes that trade places
//                  under a mirror (left / right arm of a human-parsing set) are read from their partner's channel; instances of
//                  their own (MsPermuted<MsArgs>), so the ones without a table compile from unchanged text.
//                  cseg_ms_fuse_argmax_weighted (ms_test_depth, reference :426-475): the term's scalar weight becomes a per-pixel one,
//                      v = v + table[i][bins[y,x]] * (U(a_i)[y,x] + U(b_i)[y,W-1-x])
//                  read from global memory ahead of the class loop; instances of their own again (MsWeighted<MsArgs>).
// lut_u16_u8       dst[i] = lut[src[i]], one thread per element: the depth bin of a pixel is a function of its uint16 disparity alone,
//                  so the host evaluates the reference's float64 statements once over all 65 536 values and the device looks them up
//                  (64 KB, L2-resident). No arithmetic on the device: the binning is exact by construction.
// confusion_*      integer counts, exact. K <= 128: per-block histogram of K*K 32-bit bins in LDS, non-zero bins flushed with one
//                  64-bit global atomic per bin and block. Above: lanes that hold runs of equal (gt, pred) pairs -- neighbouring
//                  pixels mostly do -- are merged with a segmented scan over the wave, one global atomic per run.
#include "cseg_ms_fuse.h"        // ms_fuse_kernel, shared with ms_eval_ragged.hip

namespace {

constexpr int CONF_LDS_K = 128;          // K*K*4 bytes of LDS: 64 KB at 128

__global__ __launch_bounds__(256) void lut_u16_u8_kernel(const uint16_t* __restrict__ src, long n, const uint8_t* __restrict__ lut,
                                                         uint8_t* __restrict__ dst) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = lut[src[i]];     // a uint16 indexes all of the 65 536 entries and nothing else
}

// bin of one pixel under RunningScore._fast_hist's mask, or -1
__device__ __forceinline__ int conf_bin(const uint8_t* pred, const int64_t* target, long i, int K, int ignore_index) {
    const int64_t t = target[i];
    const int pr = pred[i];
    return (t >= 0 && t < K && pr < K && t != (int64_t)ignore_index) ? (int)t * K + pr : -1;
}

// grid-stride; dynamic LDS = K*K unsigned
__global__ __launch_bounds__(256) void confusion_lds_kernel(const uint8_t* __restrict__ pred, const int64_t* __restrict__ target,
                                                            long N, int K, int ignore_index,
                                                            unsigned long long* __restrict__ confusion) {
    extern __shared__ unsigned conf_hist[];
    const int bins = K * K;
    for (int e = threadIdx.x; e < bins; e += 256) conf_hist[e] = 0u;
    __syncthreads();
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long)gridDim.x * 256) {
        const int bin = conf_bin(pred, target, i, K, ignore_index);
        if (bin >= 0) atomicAdd(&conf_hist[bin], 1u);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < bins; e += 256) {
        const unsigned c = conf_hist[e];
        if (c) atomicAdd(&confusion[e], (unsigned long long)c);
    }
}

// every lane of a wave takes part in every shuffle: the loop bound is rounded up to whole blocks
__global__ __launch_bounds__(256) void confusion_global_kernel(const uint8_t* __restrict__ pred, const int64_t* __restrict__ target,
                                                               long N, int K, int ignore_index,
                                                               unsigned long long* __restrict__ confusion) {
    const int lane = threadIdx.x & 63;
    const long step = (long)gridDim.x * 256;
    const long rounds = (N + step - 1) / step;
    for (long r = 0; r < rounds; ++r) {
        const long i = r * step + (long)blockIdx.x * 256 + threadIdx.x;
        const int bin = i < N ? conf_bin(pred, target, i, K, ignore_index) : -1;
        // segmented inclusive scan of ones over runs of equal bins
        const int prev = __shfl_up(bin, 1, 64);
        int head = (lane == 0 || prev != bin) ? 1 : 0;
        int cnt = 1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int c_o = __shfl_up(cnt, o, 64);
            const int h_o = __shfl_up(head, o, 64);
            if (lane >= o && !head) { cnt += c_o; head = h_o; }
        }
        const int next = __shfl(bin, (lane + 1) & 63, 64);
        const bool tail = lane == 63 || next != bin;
        if (tail && bin >= 0) atomicAdd(&confusion[bin], (unsigned long long)cnt);
    }
}

}  // namespace

extern "C" int cseg_ms_fuse_argmax_perm(int n_terms, const float* const* plain, const float* const* flipped, const int* hs,
                                        const int* ws, const float* weights, const uint8_t* perm, int B, int K, int H, int W,
                                        uint8_t* pred, float* fused, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(n_terms >= 1 && n_terms <= MS_MAX_TERMS, "ms_fuse_argmax: %d terms (1 to %d are supported)", n_terms, MS_MAX_TERMS);
    CSEG_REQUIRE(plain && hs && ws && weights, "ms_fuse_argmax: null term arrays");
    CSEG_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0, "ms_fuse_argmax: empty shape");
    CSEG_REQUIRE(K <= MS_MAX_K, "ms_fuse_argmax: %d classes (the prediction is one byte; at most %d)", K, MS_MAX_K);
    CSEG_REQUIRE(pred || fused, "ms_fuse_argmax: both outputs are null");
    CSEG_REQUIRE((long)B * H * W < 2147483647L, "ms_fuse_argmax: %d x %d x %d output pixels do not fit 31 bits", B, H, W);
    MsArgs A;
    A.n = n_terms; A.B = B; A.K = K; A.H = H; A.W = W;
    for (int i = 0; i < MS_MAX_TERMS; ++i) {
        MsTerm& t = A.t[i];
        t.a = nullptr; t.b = nullptr; t.h = 1; t.w = 1; t.sy = 0.f; t.sx = 0.f; t.wt = 0.f;
        if (i >= n_terms) continue;
        CSEG_REQUIRE(plain[i], "ms_fuse_argmax: term %d has no plain map", i);
        CSEG_REQUIRE(hs[i] > 0 && ws[i] > 0, "ms_fuse_argmax: term %d is empty (%d x %d)", i, hs[i], ws[i]);
        CSEG_REQUIRE((long)hs[i] * ws[i] < 2147483647L, "ms_fuse_argmax: term %d is too large (%d x %d)", i, hs[i], ws[i]);
        t.a = plain[i];
        t.b = flipped ? flipped[i] : nullptr;
        t.h = hs[i]; t.w = ws[i];
        t.sy = ac_scale(hs[i], H); t.sx = ac_scale(ws[i], W);
        t.wt = weights[i];
    }
    const unsigned blocks = (unsigned)(((long)B * H * W + 255) / 256);
#define LAUNCH(NT, ARGS) hipLaunchKernelGGL((ms_fuse_kernel<NT, decltype(ARGS)>), dim3(blocks), dim3(256), 0, stream, ARGS, pred, fused)
#define LAUNCH_BY_TERMS(ARGS)           \
    do {                                \
        if (n_terms <= 1) LAUNCH(1, ARGS);      \
        else if (n_terms <= 2) LAUNCH(2, ARGS); \
        else if (n_terms <= 4) LAUNCH(4, ARGS); \
        else LAUNCH(8, ARGS);           \
    } while (0)
    if (perm) {                          // everything is checked before the launch: a refused table launches nothing
        int at = 0, val = 0;
        const char* fault = ms_perm_fault(perm, K, &at, &val);
        CSEG_REQUIRE(!fault, "ms_fuse_argmax: perm[%d] = %d %s (perm must be a permutation of the %d classes)", at, val, fault, K);
        bool any_flipped = false;
        for (int i = 0; i < n_terms; ++i) any_flipped = any_flipped || A.t[i].b;
        CSEG_REQUIRE(any_flipped, "ms_fuse_argmax: a channel permutation was given but no term has a flipped map to apply it to");
        MsPermuted<MsArgs> P;
        static_cast<MsArgs&>(P) = A;
        P.perm.fill(perm, K);
        LAUNCH_BY_TERMS(P);
    } else {
        LAUNCH_BY_TERMS(A);
    }
#undef LAUNCH_BY_TERMS
#undef LAUNCH
    CSEG_CHECK_LAUNCH("ms_fuse_kernel");
    return 1;
}

extern "C" int cseg_ms_fuse_argmax(int n_terms, const float* const* plain, const float* const* flipped, const int* hs,
                                   const int* ws, const float* weights, int B, int K, int H, int W, uint8_t* pred,
                                   float* fused, cseg_stream_t stream_) {
    return cseg_ms_fuse_argmax_perm(n_terms, plain, flipped, hs, ws, weights, nullptr, B, K, H, W, pred, fused, stream_);
}

extern "C" int cseg_ms_fuse_argmax_weighted(int n_terms, const float* const* plain, const float* const* flipped, const int* hs,
                                            const int* ws, const float* weights, const uint8_t* bins, const float* table, int nbins,
                                            int B, int K, int H, int W, uint8_t* pred, float* fused, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(n_terms >= 1 && n_terms <= MS_MAX_TERMS, "ms_fuse_argmax_weighted: n_terms = %d (1 to %d are supported)", n_terms,
                 MS_MAX_TERMS);
    CSEG_REQUIRE(plain && hs && ws, "ms_fuse_argmax_weighted: null term arrays");
    CSEG_REQUIRE(B > 0 && H > 0 && W > 0, "ms_fuse_argmax_weighted: empty shape");
    CSEG_REQUIRE(K >= 1 && K <= MS_MAX_K, "ms_fuse_argmax_weighted: K = %d classes (the prediction is one byte; 1 to %d)", K, MS_MAX_K);
    CSEG_REQUIRE(nbins >= 1 && nbins <= MS_MAX_BINS, "ms_fuse_argmax_weighted: nbins = %d (1 to %d are supported)", nbins, MS_MAX_BINS);
    CSEG_REQUIRE(bins, "ms_fuse_argmax_weighted: bins is null");
    CSEG_REQUIRE(table, "ms_fuse_argmax_weighted: table is null");
    CSEG_REQUIRE(pred || fused, "ms_fuse_argmax_weighted: both outputs (pred, fused) are null");
    CSEG_REQUIRE((long)B * H * W < 2147483647L, "ms_fuse_argmax_weighted: %d x %d x %d output pixels do not fit 31 bits", B, H, W);
    MsWeighted<MsArgs> A;
    A.n = n_terms; A.B = B; A.K = K; A.H = H; A.W = W;
    A.pw.bins = bins; A.pw.table = table; A.pw.nbins = nbins;
    for (int i = 0; i < MS_MAX_TERMS; ++i) {
        MsTerm& t = A.t[i];
        t.a = nullptr; t.b = nullptr; t.h = 1; t.w = 1; t.sy = 0.f; t.sx = 0.f; t.wt = 0.f;
        if (i >= n_terms) continue;
        CSEG_REQUIRE(plain[i], "ms_fuse_argmax_weighted: term %d has no plain map", i);
        CSEG_REQUIRE(hs[i] > 0 && ws[i] > 0, "ms_fuse_argmax_weighted: term %d is empty (%d x %d)", i, hs[i], ws[i]);
        CSEG_REQUIRE((long)hs[i] * ws[i] < 2147483647L, "ms_fuse_argmax_weighted: term %d is too large (%d x %d)", i, hs[i], ws[i]);
        // the term's weight is table[i][bin]; a scalar weight beside it would be a second factor that the reference does not have
        CSEG_REQUIRE(!weights || weights[i] == 1.f, "ms_fuse_argmax_weighted: weights[%d] = %g (the weights come from table; pass NULL or "
                     "ones)", i, (double)(weights ? weights[i] : 1.f));
        t.a = plain[i];
        t.b = flipped ? flipped[i] : nullptr;
        t.h = hs[i]; t.w = ws[i];
        t.sy = ac_scale(hs[i], H); t.sx = ac_scale(ws[i], W);
        t.wt = 1.f;
    }
    const unsigned blocks = (unsigned)(((long)B * H * W + 255) / 256);
#define LAUNCH(NT) hipLaunchKernelGGL((ms_fuse_kernel<NT, MsWeighted<MsArgs>>), dim3(blocks), dim3(256), 0, stream, A, pred, fused)
    if (n_terms <= 1) LAUNCH(1);
    else if (n_terms <= 2) LAUNCH(2);
    else if (n_terms <= 4) LAUNCH(4);
    else LAUNCH(8);
#undef LAUNCH
    CSEG_CHECK_LAUNCH("ms_fuse_kernel (weighted)");
    return 1;
}

extern "C" int cseg_lut_u16_u8(const uint16_t* src, long n, const uint8_t* lut, uint8_t* dst, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(n >= 0 && n < 2147483648L, "lut_u16_u8: n = %ld elements (fewer than 2^31 are supported)", n);
    if (n == 0) return 1;
    CSEG_REQUIRE(src && lut && dst, "lut_u16_u8: null pointer");
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(lut_u16_u8_kernel, dim3(blocks), dim3(256), 0, stream, src, n, lut, dst);
    CSEG_CHECK_LAUNCH("lut_u16_u8_kernel");
    return 1;
}

extern "C" int cseg_confusion_update(const uint8_t* pred, const int64_t* target, long N, int K, int ignore_index,
                                     int64_t* confusion, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(pred && target && confusion, "confusion_update: null pointer");
    CSEG_REQUIRE(K > 0 && K <= 32768, "confusion_update: %d classes", K);
    CSEG_REQUIRE(N >= 0 && N < 2147483648L, "confusion_update: %ld pixels in one call (fewer than 2^31 are supported)", N);
    if (N == 0) return 1;
    unsigned long long* conf = reinterpret_cast<unsigned long long*>(confusion);
    // 16 pixels per thread and at most 1024 blocks: a block's flush of its LDS bins is amortised over >= 4096 pixels
    const long want = (N + 256L * 16 - 1) / (256L * 16);
    const unsigned blocks = (unsigned)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
    if (K <= CONF_LDS_K) {
        hipLaunchKernelGGL(confusion_lds_kernel, dim3(blocks), dim3(256), sizeof(unsigned) * K * K, stream, pred, target, N, K,
                           ignore_index, conf);
        CSEG_CHECK_LAUNCH("confusion_lds_kernel");
    } else {
        hipLaunchKernelGGL(confusion_global_kernel, dim3(blocks), dim3(256), 0, stream, pred, target, N, K, ignore_index, conf);
        CSEG_CHECK_LAUNCH("confusion_global_kernel");
    }
    return 1;
}
