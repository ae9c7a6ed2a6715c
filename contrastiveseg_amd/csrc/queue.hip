// Memory-bank (segment / pixel queue) update kernels.
// Reference: segmentor/trainer_contrastive.py:102-138 (_dequeue_and_enqueue). The Python loop over
// (image, class) with unique / nonzero / mean / normalize per pair becomes: one histogram, one pass over the key
// map that accumulates every class at once, and two small row writers. Pointer arithmetic and the CPU randperm
// stay on the host (contrastiveseg_amd/segmentor/trainer_contrastive.py) -- unless contrast.device_bank is on: cseg_queue_enqueue_device,
// at the end of this file, does them on the device too. HBM-bound; no MFMA.
#include "cseg_common.h"
#include "cseg_sampling.h"

namespace {

__global__ __launch_bounds__(256) void queue_count_kernel(const int64_t* __restrict__ labels, int H, int W, int stride,
                                                          int Hs, int Ws, int K, int32_t* __restrict__ counts) {
    extern __shared__ int hist[];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < K; i += 256) hist[i] = 0;
    __syncthreads();
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < Hs * Ws) {
        const int ys = q / Ws, xs = q - ys * Ws;
        const int64_t l = labels[((size_t)b * H + (size_t)ys * stride) * W + (size_t)xs * stride];
        if (l >= 0 && l < K) atomicAdd(&hist[(int)l], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K; i += 256)
        if (hist[i]) atomicAdd(&counts[(size_t)b * K + i], hist[i]);
}

// One wave per (image, channel): lanes stride over the Q positions (coalesced), every lane keeps one private
// accumulator per class of the current chunk of 32 classes; fixed-order wave reduction => deterministic sums.
__global__ __launch_bounds__(256) void queue_class_sums_kernel(const float* __restrict__ keys,
                                                               const int64_t* __restrict__ labels, int D, int Pk,
                                                               int H, int W, int stride, int Hs, int Ws, int K,
                                                               float* __restrict__ sums) {
    const int b = blockIdx.y;
    const int dch = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (dch >= D) return;
    const int Q = Hs * Ws;
    const float* kp = keys + ((size_t)b * D + dch) * Pk;
    for (int c0 = 0; c0 < K; c0 += 32) {
        float acc[32];
#pragma unroll
        for (int c = 0; c < 32; ++c) acc[c] = 0.f;
        for (int q = lane; q < Q; q += 64) {
            const int ys = q / Ws, xs = q - ys * Ws;
            const int l = (int)labels[((size_t)b * H + (size_t)ys * stride) * W + (size_t)xs * stride] - c0;
            const float v = kp[q];
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] += (l == c) ? v : 0.f;
        }
#pragma unroll
        for (int c = 0; c < 32; ++c) {
            const float s = wave_sum(acc[c]);
            if (lane == 0 && c0 + c < K) sums[((size_t)b * K + c0 + c) * D + dch] = s;
        }
    }
}

// block per job: mean, L2 normalise (F.normalize eps 1e-12), write one bank row
__global__ __launch_bounds__(256) void queue_write_segments_kernel(const float* __restrict__ sums,
                                                                   const int32_t* __restrict__ counts,
                                                                   const int32_t* __restrict__ job_img,
                                                                   const int32_t* __restrict__ job_cls,
                                                                   const int32_t* __restrict__ job_dst, int K, int D,
                                                                   float* __restrict__ segq, int ms) {
    __shared__ float red[4];
    const int j = blockIdx.x;
    const int b = job_img[j], c = job_cls[j], row = job_dst[j];
    const float inv = 1.f / (float)counts[(size_t)b * K + c];
    const float* src = sums + ((size_t)b * K + c) * D;
    float ss = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) { const float v = src[d] * inv; ss += v * v; }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(red[0] + red[1] + red[2] + red[3]), 1e-12f);
    float* dst = segq + ((size_t)c * ms + row) * D;
    for (int d = threadIdx.x; d < D; d += 256) dst[d] = src[d] * inv / nrm;
}

// wave per row: gather one pixel's channel vector from the NCHW key map, normalise, write
__global__ __launch_bounds__(256) void queue_write_pixels_kernel(const float* __restrict__ keys, int D, int Pk,
                                                                 const int32_t* __restrict__ src_img,
                                                                 const int32_t* __restrict__ src_pos,
                                                                 const int32_t* __restrict__ dst_cls,
                                                                 const int32_t* __restrict__ dst_row, int n_rows,
                                                                 float* __restrict__ pixq, int ms) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rows) return;
    const float* src = keys + (size_t)src_img[r] * D * Pk + src_pos[r];
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) { const float v = src[(size_t)d * Pk]; ss += v * v; }
    const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    float* dst = pixq + ((size_t)dst_cls[r] * ms + dst_row[r]) * D;
    for (int d = lane; d < D; d += 64) dst[d] = src[(size_t)d * Pk] / nrm;
}

}  // namespace

extern "C" int cseg_queue_count(const int64_t* labels, int B, int H, int W, int stride, int K, int32_t* counts,
                                cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(stride >= 1 && B > 0 && K > 0, "queue_count: bad arguments");
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    if (hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)B * K, stream) != hipSuccess) {
        cseg_set_error("queue_count: memset failed");
        return 0;
    }
    dim3 grid((Hs * Ws + 255) / 256, B);
    hipLaunchKernelGGL(queue_count_kernel, grid, dim3(256), sizeof(int) * K, stream, labels, H, W, stride, Hs, Ws, K,
                       counts);
    CSEG_CHECK_LAUNCH("queue_count_kernel");
    return 1;
}

extern "C" int cseg_queue_class_sums(const float* keys, const int64_t* labels, int B, int D, int Pk, int H, int W,
                                     int stride, int K, float* sums, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(stride >= 1 && B > 0 && K > 0 && D > 0, "queue_class_sums: bad arguments");
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    // the reference indexes keys[b].view(D,-1) with positions of the strided label map (:111-120)
    CSEG_REQUIRE(Hs * Ws <= Pk, "queue_class_sums: strided label map (%d) larger than key map (%d)", Hs * Ws, Pk);
    dim3 grid((D + 3) / 4, B);
    hipLaunchKernelGGL(queue_class_sums_kernel, grid, dim3(256), 0, stream, keys, labels, D, Pk, H, W, stride, Hs, Ws,
                       K, sums);
    CSEG_CHECK_LAUNCH("queue_class_sums_kernel");
    return 1;
}

extern "C" int cseg_queue_write_segments(const float* sums, const int32_t* counts, const int32_t* job_img,
                                         const int32_t* job_cls, const int32_t* job_dst_row, int n_jobs, int K, int D,
                                         float* segment_queue, int ms, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_jobs <= 0) return 1;
    hipLaunchKernelGGL(queue_write_segments_kernel, dim3(n_jobs), dim3(256), 0, stream, sums, counts, job_img, job_cls,
                       job_dst_row, K, D, segment_queue, ms);
    CSEG_CHECK_LAUNCH("queue_write_segments_kernel");
    return 1;
}

extern "C" int cseg_queue_write_pixels(const float* keys, int B, int D, int Pk, const int32_t* src_img,
                                       const int32_t* src_pos, const int32_t* dst_cls, const int32_t* dst_row,
                                       int n_rows, float* pixel_queue, int ms, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    (void)B;
    if (n_rows <= 0) return 1;
    hipLaunchKernelGGL(queue_write_pixels_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, stream, keys, D, Pk, src_img,
                       src_pos, dst_cls, dst_row, n_rows, pixel_queue, ms);
    CSEG_CHECK_LAUNCH("queue_write_pixels_kernel");
    return 1;
}

// ---------------------------------------------------------------------------------------------------------
// The whole enqueue on the device (contrast.device_bank): what plan_enqueue of segmentor/trainer_contrastive.py
// does on the host -- the walk over the (image, class >= 1) pairs, the pointer arithmetic, one torch.randperm per pair and the
// last-writer-wins resolution -- as a planner block, the generator kernel of sampling.hip and one thread per randperm call. Nothing
// is read back and no value of the host depends on the data.
//
//   fill_zero_kernel            counts <- 0 (a kernel, not hipMemsetAsync: DESIGN.md section 20.6)
//   queue_count_kernel, queue_class_sums_kernel   as above
//   enqueue_plan_kernel         one block. Pair slot p = b * (K - 1) + (lb - 1): ascending p IS the reference's order (image-major,
//                               class ascending). Block prefix sum of max(n - 1, 0) over the live pairs = offset of each call's
//                               first draw, and the step's total (header[3], what cseg_mt_draw generates). One thread per class
//                               walks the images serially with the reference's pointer arithmetic, then stores the new pointers.
//   (cseg_mt_draw)
//   enqueue_pick_kernel         one thread per pair: the truncated Fisher-Yates of sampling.hip's pick_kernel, k = min(n, freq)
//   enqueue_write_segments_kernel / enqueue_write_pixels_kernel   the statements of the two writers above behind the plan: a write
//                               is dropped when a LATER image's pair of the same class covers the same bank row, so every row has
//                               at most one writer and no ordering between blocks is relied on.
// plan [B*(K-1)][4] = {n (0: no such pair), offset of the first draw, segment row, first pixel row}; k = min(n, freq) is recomputed.
// ---------------------------------------------------------------------------------------------------------
namespace {

constexpr int EQ_HEADER = 8;

__global__ __launch_bounds__(256) void fill_zero_kernel(int32_t* __restrict__ p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

__device__ __forceinline__ int wrap_ptr(int64_t p, int ms) {      // a pointer buffer holds 0 <= p < ms; anything else is folded into range
    const int64_t r = p % ms;
    return (int)(r < 0 ? r + ms : r);
}

__global__ __launch_bounds__(SP_THREADS) void enqueue_plan_kernel(const int32_t* __restrict__ counts, int B, int K, int ms, int freq,
                                                                  int draw_cap, int64_t* __restrict__ seg_ptr,
                                                                  int64_t* __restrict__ pix_ptr, int32_t* __restrict__ plan,
                                                                  int32_t* __restrict__ header) {
    __shared__ int red[SP_THREADS / 64];
    const int tid = threadIdx.x;
    const int Kp = K - 1, cap = B * Kp;
    const int per = (cap + SP_THREADS - 1) / SP_THREADS;
    const int p_lo = min(cap, tid * per), p_hi = min(cap, p_lo + per);
    int dr = 0, live = 0, rows = 0;
    for (int p = p_lo; p < p_hi; ++p) {
        const int b = p / Kp, lb = 1 + p - b * Kp;
        const int n = counts[b * K + lb];
        dr += draws_of(n);
        live += n > 0 ? 1 : 0;
        rows += min(n, freq);
    }
    int total, n_live, n_rows;
    int off = block_excl_scan(dr, red, tid, &total);
    block_excl_scan(live, red, tid, &n_live);
    block_excl_scan(rows, red, tid, &n_rows);
    for (int p = p_lo; p < p_hi; ++p) {
        const int b = p / Kp, lb = 1 + p - b * Kp;
        const int n = counts[b * K + lb];
        plan[4 * p] = n;
        plan[4 * p + 1] = off;
        off += draws_of(n);
    }
    // trainer_contrastive.py:plan_enqueue, one class per thread (classes are independent), images in order
    for (int lb = 1 + tid; lb < K; lb += SP_THREADS) {
        int sp = wrap_ptr(seg_ptr[lb], ms), pp = wrap_ptr(pix_ptr[lb], ms);
        for (int b = 0; b < B; ++b) {
            const int n = counts[b * K + lb];
            const int p = b * Kp + lb - 1;
            int srow = 0, prow = 0;
            if (n > 0) {
                srow = sp;
                sp = (sp + 1) % ms;
                const int k = min(n, freq);
                if (pp + k >= ms) {
                    prow = ms - k;
                    pp = 0;
                } else {
                    prow = pp;
                    pp = (pp + 1) % ms;         // + 1, not + k: as the reference
                }
            }
            plan[4 * p + 2] = srow;
            plan[4 * p + 3] = prow;
        }
        seg_ptr[lb] = sp;                       // after the rows of this class are in the plan
        pix_ptr[lb] = pp;
    }
    if (tid == 0) {
        header[0] = n_live;
        header[1] = n_rows;
        header[2] = 0;
        header[3] = min(total, draw_cap);       // (sum max(n - 1, 0) <= B * Hs * Ws = draw_cap for counts of queue_count_kernel)
        header[4] = 0; header[5] = 0; header[6] = 0; header[7] = 0;
    }
}

// fy_ws [B*(K-1)][freq][2]: the touched positions of the permutation and what they hold; pos [B*(K-1)][freq]: the first k values of
// the pair's permutation = columns of keys[b].view(D, -1)
__global__ __launch_bounds__(SP_THREADS) void enqueue_pick_kernel(const int32_t* __restrict__ plan, const uint32_t* __restrict__ draws,
                                                                  int cap, int freq, int draw_cap, int32_t* __restrict__ fy_ws,
                                                                  int32_t* __restrict__ pos) {
    const int p = blockIdx.x * SP_THREADS + threadIdx.x;
    if (p >= cap) return;
    const int n = plan[4 * p];
    if (n <= 0) return;
    const int k = min(n, freq);
    const int steps = draws_of(n), kk = min(k, steps);
    const int d0 = plan[4 * p + 1];
    if (d0 < 0 || d0 + steps > draw_cap) return;             // cannot happen for a plan of enqueue_plan_kernel
    const uint32_t* dw = draws + d0;
    int32_t* ws = fy_ws + 2 * (size_t)p * freq;
    int32_t* out = pos + (size_t)p * freq;
    int cnt = 0;
    for (int i = 0; i < kk; ++i) {
        const int zi = i + (int)(dw[i] % (uint32_t)(n - i));
        int vi = i, vj = zi, at = -1;
        for (int t = 0; t < cnt; ++t) {
            const int q = ws[2 * t], val = ws[2 * t + 1];
            if (q == i) vi = val;
            if (q == zi) { vj = val; at = t; }
        }
        out[i] = vj;                                    // r[i] after the swap
        if (at < 0) {
            at = cnt++;
            ws[2 * at] = zi;
        }
        ws[2 * at + 1] = vi;
    }
    if (k > kk) {                                       // k == n: the last entry is what is left at n - 1
        int vl = n - 1;
        for (int t = 0; t < cnt; ++t)
            if (ws[2 * t] == n - 1) vl = ws[2 * t + 1];
        out[kk] = vl;
    }
}

// block per pair slot: queue_write_segments_kernel behind the plan
__global__ __launch_bounds__(256) void enqueue_write_segments_kernel(const float* __restrict__ sums, const int32_t* __restrict__ counts,
                                                                     const int32_t* __restrict__ plan, int B, int K, int D,
                                                                     float* __restrict__ segq, int ms) {
    __shared__ float red[4];
    const int Kp = K - 1;
    const int j = blockIdx.x;
    const int b = j / Kp, c = 1 + j - b * Kp;
    if (plan[4 * j] <= 0) return;
    const int row = plan[4 * j + 2];
    if (row < 0 || row >= ms) return;
    for (int b2 = b + 1; b2 < B; ++b2) {                // a later image writes this row: its write is the one that stays
        const int j2 = b2 * Kp + c - 1;
        if (plan[4 * j2] > 0 && plan[4 * j2 + 2] == row) return;
    }
    const float inv = 1.f / (float)counts[(size_t)b * K + c];
    const float* src = sums + ((size_t)b * K + c) * D;
    float ss = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) { const float v = src[d] * inv; ss += v * v; }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(red[0] + red[1] + red[2] + red[3]), 1e-12f);
    float* dst = segq + ((size_t)c * ms + row) * D;
    for (int d = threadIdx.x; d < D; d += 256) dst[d] = src[d] * inv / nrm;
}

// wave per (pair slot, i < freq): queue_write_pixels_kernel behind the plan
__global__ __launch_bounds__(256) void enqueue_write_pixels_kernel(const float* __restrict__ keys, int D, int Pk,
                                                                   const int32_t* __restrict__ plan, const int32_t* __restrict__ pos,
                                                                   int B, int K, int freq, float* __restrict__ pixq, int ms) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int Kp = K - 1;
    if (r >= B * Kp * freq) return;
    const int j = r / freq, i = r - j * freq;
    const int n = plan[4 * j];
    if (i >= min(n, freq)) return;
    const int b = j / Kp, c = 1 + j - b * Kp;
    const int row = plan[4 * j + 3] + i;
    const int sp = pos[r];
    if (row < 0 || row >= ms || sp < 0 || sp >= Pk) return;
    for (int b2 = b + 1; b2 < B; ++b2) {
        const int j2 = b2 * Kp + c - 1;
        const int n2 = plan[4 * j2], r2 = plan[4 * j2 + 3];
        if (n2 > 0 && row >= r2 && row < r2 + min(n2, freq)) return;
    }
    const float* src = keys + (size_t)b * D * Pk + sp;
    float ss = 0.f;
    for (int d = lane; d < D; d += 64) { const float v = src[(size_t)d * Pk]; ss += v * v; }
    const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
    float* dst = pixq + ((size_t)c * ms + row) * D;
    for (int d = lane; d < D; d += 64) dst[d] = src[(size_t)d * Pk] / nrm;
}

struct EnqueueLayout { size_t counts, header, plan, pos, fy, draws, total; };

inline EnqueueLayout enqueue_layout(int B, int K, int Q, int freq) {
    EnqueueLayout l;
    const size_t cap = (size_t)B * (K - 1);
    l.counts = 0;
    l.header = l.counts + (size_t)B * K;
    l.plan = l.header + EQ_HEADER;
    l.pos = l.plan + 4 * cap;
    l.fy = l.pos + cap * freq;
    l.draws = l.fy + 2 * cap * freq;
    l.total = l.draws + (size_t)B * Q;
    return l;
}

}  // namespace

extern "C" int cseg_mt_draw(uint32_t* rng_state, const int32_t* header, uint32_t* draws, int cap, cseg_stream_t stream);

extern "C" size_t cseg_queue_enqueue_ws_ints(int B, int K, int H, int W, int stride, int pixel_update_freq) {
    if (B <= 0 || K < 2 || H <= 0 || W <= 0 || stride < 1 || pixel_update_freq < 1) return 0;
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    return enqueue_layout(B, K, Hs * Ws, pixel_update_freq).total;
}

extern "C" int cseg_queue_enqueue_device(const float* keys, const int64_t* labels, int B, int D, int Pk, int H, int W, int stride,
                                         int K, int ms, int pixel_update_freq, float* segment_queue, int64_t* segment_queue_ptr,
                                         float* pixel_queue, int64_t* pixel_queue_ptr, uint32_t* rng_state, float* sums,
                                         int32_t* ws, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int freq = pixel_update_freq;
    CSEG_REQUIRE(stride >= 1 && B > 0 && K >= 2 && D > 0 && H > 0 && W > 0, "queue_enqueue_device: bad arguments");
    CSEG_REQUIRE(ms > 0 && freq >= 1 && freq <= ms, "queue_enqueue_device: pixel_update_freq=%d must be in [1, memory_size=%d]", freq, ms);
    const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
    CSEG_REQUIRE(Hs * Ws <= Pk, "queue_enqueue_device: strided label map (%d) larger than key map (%d)", Hs * Ws, Pk);
    CSEG_REQUIRE((size_t)B * Hs * Ws < ((size_t)1 << 31) && (size_t)B * (K - 1) * freq < ((size_t)1 << 30),
                 "queue_enqueue_device: B*Hs*Ws or B*(K-1)*freq overflows int32");
    const int Q = Hs * Ws, cap = B * (K - 1);
    const EnqueueLayout l = enqueue_layout(B, K, Q, freq);
    int32_t* counts = ws + l.counts;
    int32_t* header = ws + l.header;
    int32_t* plan = ws + l.plan;
    int32_t* pos = ws + l.pos;
    int32_t* fy = ws + l.fy;
    uint32_t* draws = reinterpret_cast<uint32_t*>(ws + l.draws);
    hipLaunchKernelGGL(fill_zero_kernel, dim3((B * K + 255) / 256), dim3(256), 0, stream, counts, B * K);
    CSEG_CHECK_LAUNCH("fill_zero_kernel");
    hipLaunchKernelGGL(queue_count_kernel, dim3((Q + 255) / 256, B), dim3(256), sizeof(int) * K, stream, labels, H, W, stride, Hs, Ws,
                       K, counts);
    CSEG_CHECK_LAUNCH("queue_count_kernel");
    hipLaunchKernelGGL(queue_class_sums_kernel, dim3((D + 3) / 4, B), dim3(256), 0, stream, keys, labels, D, Pk, H, W, stride, Hs, Ws,
                       K, sums);
    CSEG_CHECK_LAUNCH("queue_class_sums_kernel");
    hipLaunchKernelGGL(enqueue_plan_kernel, dim3(1), dim3(SP_THREADS), 0, stream, counts, B, K, ms, freq, B * Q, segment_queue_ptr,
                       pixel_queue_ptr, plan, header);
    CSEG_CHECK_LAUNCH("enqueue_plan_kernel");
    if (!cseg_mt_draw(rng_state, header, draws, B * Q, stream_)) return 0;
    hipLaunchKernelGGL(enqueue_pick_kernel, dim3((cap + SP_THREADS - 1) / SP_THREADS), dim3(SP_THREADS), 0, stream, plan, draws, cap,
                       freq, B * Q, fy, pos);
    CSEG_CHECK_LAUNCH("enqueue_pick_kernel");
    hipLaunchKernelGGL(enqueue_write_segments_kernel, dim3(cap), dim3(256), 0, stream, sums, counts, plan, B, K, D, segment_queue, ms);
    CSEG_CHECK_LAUNCH("enqueue_write_segments_kernel");
    hipLaunchKernelGGL(enqueue_write_pixels_kernel, dim3((cap * freq + 3) / 4), dim3(256), 0, stream, keys, D, Pk, plan, pos, B, K, freq,
                       pixel_queue, ms);
    CSEG_CHECK_LAUNCH("enqueue_write_pixels_kernel");
    return 1;
}
