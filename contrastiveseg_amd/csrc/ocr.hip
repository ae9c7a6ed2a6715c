// The object-context block of the OCR models (lib/models/modules/spatial_ocr_block.py): soft region pooling (SpatialGather_Module) and
// the pixel -> region attention (ObjectAttentionBlock2D), forward and backward, as exact-fp32 GEMMs on v_mfma_f32_32x32x2_f32 with the two
// softmaxes fused into their loaders / epilogues. The operators have the shapes of csrc/cls1x1_wide.hip (see there for the operand maps of
// the instruction: lane l, r = l & 31, h = l >> 5; A[i = r][k = h], B[k = h][j = r], D row d_row(v, h) in register v, column r):
//   gather    ctx[b][c][k]  = sum_p s[b][k][p] feats[b][c][p]           s = softmax_p(scale probs)      (weight-gradient shape)
//             g[b][k][p]    = sum_c dctx[b][c][k] feats[b][c][p]         dprobs = scale s (g - sum_p s g)  (forward shape)
//             dfeats[b][c][p] = sum_k dctx[b][c][k] s[b][k][p]                                            (backward-data shape)
//   attention l[b][k][p]    = sum_c key[b][c][k] q[b][c][p]              a = softmax_k(scale l)          (forward shape)
//             out[b][c][p]  = sum_k value[b][c][k] a[b][k][p]                                             (backward-data shape)
//             dA = value^T dout, delta = sum_k a dA, dl = scale a (dA - delta), dq = key dl, dkey = q dl^T, dvalue = dout a^T
// The per-image matrices key / value / ctx / dctx are [B][C][K] as the modules hold them (no pad columns in memory: the loaders put zeros
// into the columns K .. KP of the LDS tiles), KP = K rounded up to whole 32-class tiles, at least 64; NT = KP / 32 is the template parameter.
// Forward: s and a never reach memory. The gather keeps max and sum exp of every (b, k) row (2 B K floats), the attention max and sum exp of
// every pixel (2 B P floats); the backward passes recompute the probabilities from them.
// All sums in a fixed order (no atomics): deterministic. Any P and any C: ragged tiles load zeros and skip the stores.
#include "cseg_common.h"
#include "cseg_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CC = 32;                 // channels per LDS chunk / tile
constexpr int PXB = 128;               // pixels per block (pixel-owning kernels): 4 waves x 32

// row of D held in register v by lane half h
__device__ __forceinline__ int d_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// a chunk of 32 channels x KP classes of a [C][K] matrix, coalesced along K, zeros beyond C and K: element tid + 256 q
template <int NT>
__device__ __forceinline__ void fetch_chunk(const float* __restrict__ wp, int c0, int C, int K, int tid, float (&wreg)[NT * 4]) {
    constexpr int KP = NT * 32;
#pragma unroll
    for (int q = 0; q < NT * 4; ++q) {
        const int idx = tid + 256 * q, c = c0 + idx / KP, k = idx % KP;
        wreg[q] = (c < C && k < K) ? wp[(size_t)c * K + k] : 0.f;
    }
}

// acc[t][v] = sum_c w[c][32 t + d_row(v, h)] x[c][pixel of the lane]: the loop of cls1x1_wide_fwd_kernel. x is the B operand straight
// from global memory (xp = the lane's pixel of channel 0), the matrix goes through LDS in chunks of 32 channels (pitch = 32 mod 64).
template <int NT>
__device__ __forceinline__ void gemm_over_channels(const float* __restrict__ xp, const float* __restrict__ wp, int C, int K, long P,
                                                   float* __restrict__ Ws, f32x16 (&acc)[NT]) {
    constexpr int KP = NT * 32, PITCH = (NT | 1) * 32, WREG = NT * 4;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    float wreg[WREG], xreg[CC / 2];
    auto fetch = [&](int c0) {
        fetch_chunk<NT>(wp, c0, C, K, tid, wreg);
#pragma unroll
        for (int s = 0; s < CC / 2; ++s) {
            const int c = c0 + 2 * s + h;
            xreg[s] = c < C ? xp[(size_t)c * P] : 0.f;
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < C; c0 += CC) {
        __syncthreads();                                       // the previous chunk has been consumed
#pragma unroll
        for (int q = 0; q < WREG; ++q) {
            const int idx = tid + 256 * q;
            Ws[(idx / KP) * PITCH + idx % KP] = wreg[q];
        }
        float xcur[CC / 2];
#pragma unroll
        for (int s = 0; s < CC / 2; ++s) xcur[s] = xreg[s];
        __syncthreads();
        if (c0 + CC < C) fetch(c0 + CC);                       // in flight under the chunk's 16 NT matrix instructions
        float a[NT], an[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) a[t] = Ws[h * PITCH + t * 32 + r];
#pragma unroll
        for (int s = 0; s < CC / 2; ++s) {
            if (s + 1 < CC / 2) {
#pragma unroll
                for (int t = 0; t < NT; ++t) an[t] = Ws[(2 * s + 2 + h) * PITCH + t * 32 + r];
            }
            __builtin_amdgcn_sched_barrier(0);                 // (the reads of step s + 1 stay in front of the instructions of step s)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], xcur[s], acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NT; ++t) a[t] = an[t];
        }
    }
}

// ---- pixel-owning kernel: a wave = 32 pixels with all KP classes of them in NT accumulator tiles ------------------------------------
enum { M_PLAIN = 0, M_ATTN = 1, M_ATTN_STATS = 2, M_PROB = 3, M_DLOGIT = 4 };
//   M_PLAIN       out[b][k][p] = acc                                                            (gather backward: g)
//   M_ATTN(_STATS) a = softmax over the K classes of scale acc (pad classes masked out), out[b][c][p] = sum_k aux[b][c][k] a[k]: the
//                 probabilities are the B operand of the second GEMM as they lie in the accumulators -- step (t, v) pairs the classes
//                 32 t + d_row(v, 0) and 32 t + d_row(v, 1) that the two lane halves hold; _STATS writes max and sum exp per pixel
//   M_PROB        out[b][k][p] = exp(scale acc - max) / sum from the statistics in aux       (attention backward: a)
//   M_DLOGIT      out[b][k][p] = scale a (acc - sum_k a acc), a [B][K][P] in aux              (attention backward: dl; acc = dA)
template <int NT, int MODE>
__global__ __launch_bounds__(256) void ocr_pixel_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ aux, float scale, int C, int K, long P, int tiles,
                                                        float* __restrict__ out, float* __restrict__ stats) {
    constexpr int KP = NT * 32, VP = KP + 1;                   // Vs[c][k], odd pitch: the 32 lanes of a half (c = r) read 32 banks
    __shared__ float S[CC * (KP + 32)];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long p = (long)tile * PXB + wave * 32 + r;
    const bool live = p < P;
    const long pc = live ? p : P - 1;
    f32x16 acc[NT];
    gemm_over_channels<NT>(x + (size_t)b * C * P + pc, w + (size_t)b * C * K, C, K, P, S, acc);
    if (MODE == M_PLAIN || MODE == M_PROB || MODE == M_DLOGIT) {
        float mx = 0.f, inv = 0.f, delta = 0.f;
        if (MODE == M_PROB) {
            mx = aux[(size_t)b * 2 * P + pc];
            inv = 1.f / aux[((size_t)b * 2 + 1) * P + pc];
        }
        if (MODE == M_DLOGIT) {
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int k = t * 32 + d_row(v, h);
                    delta += k < K ? aux[((size_t)b * K + k) * P + pc] * acc[t][v] : 0.f;
                }
            delta += __shfl_xor(delta, 32, 64);
        }
        if (live) {
            float* op = out + (size_t)b * K * P + p;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int k = t * 32 + d_row(v, h);
                    if (k < K) {
                        float y = acc[t][v];
                        if (MODE == M_PROB) y = __expf(scale * y - mx) * inv;
                        if (MODE == M_DLOGIT) y = scale * aux[((size_t)b * K + k) * P + p] * (y - delta);
                        op[(size_t)k * P] = y;
                    }
                }
        }
        return;
    }
    // softmax over the classes: each lane half holds half of the classes of pixel r
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            acc[t][v] *= scale;
            if (t * 32 + d_row(v, h) < K) mx = fmaxf(mx, acc[t][v]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            acc[t][v] = t * 32 + d_row(v, h) < K ? __expf(acc[t][v] - mx) : 0.f;      // a zero key column is a logit of 0, not a class
            sum += acc[t][v];
        }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] *= inv;
    if (MODE == M_ATTN_STATS && live && h == 0) {
        stats[(size_t)b * 2 * P + p] = mx;
        stats[((size_t)b * 2 + 1) * P + p] = sum;
    }
    // out[c][p] = sum_k value[c][k] a[k][p], 32 channels at a time
    const float* vp = aux + (size_t)b * C * K;
    float wreg[NT * 4];
    fetch_chunk<NT>(vp, 0, C, K, tid, wreg);
    for (int c0 = 0; c0 < C; c0 += CC) {
        __syncthreads();                                       // the previous chunk (or the last key chunk) has been consumed
#pragma unroll
        for (int q = 0; q < NT * 4; ++q) {
            const int idx = tid + 256 * q;
            S[(idx / KP) * VP + idx % KP] = wreg[q];
        }
        __syncthreads();
        if (c0 + CC < C) fetch_chunk<NT>(vp, c0 + CC, C, K, tid, wreg);
        f32x16 o;
#pragma unroll
        for (int v = 0; v < 16; ++v) o[v] = 0.f;
        float a[16], an[16];                                   // the A operands of the next class tile are read under the current one
#pragma unroll
        for (int v = 0; v < 16; ++v) a[v] = S[r * VP + d_row(v, h)];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t + 1 < NT) {
#pragma unroll
                for (int v = 0; v < 16; ++v) an[v] = S[r * VP + (t + 1) * 32 + d_row(v, h)];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = 0; v < 16; ++v) o = __builtin_amdgcn_mfma_f32_32x32x2f32(a[v], acc[t][v], o, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = 0; v < 16; ++v) a[v] = an[v];
        }
        if (live) {
            float* op = out + ((size_t)b * C + c0) * P + p;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int c = d_row(v, h);
                if (c0 + c < C) op[(size_t)c * P] = o[v];
            }
        }
    }
}

// ---- backward-data shape: dx[b][c][p] = sum_k w[b][c][k] d[b][k][p] -------------------------------------------------------------------
// The loop of cls1x1_wide_bwd_kernel (a wave = 32 pixels with their d in registers as the B operand; 32-channel tiles of w through LDS).
// SOFT: d = exp(scale probs - max[b][k]) / sum[b][k] from the row statistics (gather: dfeats).
template <int NT, bool SOFT>
__global__ __launch_bounds__(256) void ocr_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                      const float* __restrict__ rstats, float scale, int B, int C, int K, long P,
                                                      int tiles, float* __restrict__ dx) {
    constexpr int KP = NT * 32, PITCH = KP + 1, WREG = NT * 4;
    __shared__ float Wt[CC * PITCH];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long p = (long)tile * PXB + wave * 32 + r;
    const bool live = p < P;
    const long pc = live ? p : P - 1;
    float d[KP / 2];                                           // B operand of step kk: d[class 2 kk + h][pixel r]
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) {
        const int k = 2 * kk + h;
        float v = k < K ? dy[((size_t)b * K + k) * P + pc] : 0.f;
        if (SOFT && k < K) v = __expf(scale * v - rstats[(size_t)b * K + k]) / rstats[(size_t)B * K + (size_t)b * K + k];
        d[kk] = v;
    }
    const int c_tiles = (C + CC - 1) / CC;
    const int per = (c_tiles + (int)gridDim.y - 1) / (int)gridDim.y;
    const int t0 = blockIdx.y * per, t1 = min(c_tiles, t0 + per);
    const float* wp = w + (size_t)b * C * K;
    float wreg[WREG];
    if (t0 < t1) fetch_chunk<NT>(wp, t0 * CC, C, K, tid, wreg);
    for (int ct = t0; ct < t1; ++ct) {
        const int c0 = ct * CC;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < WREG; ++q) {
            const int idx = tid + 256 * q;
            Wt[(idx / KP) * PITCH + idx % KP] = wreg[q];
        }
        __syncthreads();
        if (ct + 1 < t1) fetch_chunk<NT>(wp, c0 + CC, C, K, tid, wreg);
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
        constexpr int G = 8;                                   // the A operands of the next eight steps are read under the current eight
        float a[G], an[G];
#pragma unroll
        for (int j = 0; j < G; ++j) a[j] = Wt[r * PITCH + 2 * j + h];
#pragma unroll
        for (int k0 = 0; k0 < KP / 2; k0 += G) {
            if (k0 + G < KP / 2) {
#pragma unroll
                for (int j = 0; j < G; ++j) an[j] = Wt[r * PITCH + 2 * (k0 + G + j) + h];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < G; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], d[k0 + j], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < G; ++j) a[j] = an[j];
        }
        if (live) {
            float* op = dx + ((size_t)b * C + c0) * P + p;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int c = d_row(v, h);
                if (c0 + c < C) op[(size_t)c * P] = acc[v];
            }
        }
    }
}

// ---- weight-gradient shape: o[b][c][k] = sum_p x[b][c][p] d[b][k][p] ------------------------------------------------------------------
// The loop of cls1x1_wide_wrw_kernel (block = 128 channels x all KP classes x a split of the pixels; both operands transposed through
// LDS, odd pitch: the lane = row reads of a half hit 32 banks). SOFT: d = exp(scale probs - max) / sum in the loader (gather: ctx).
constexpr int WCB = 128;               // channels per block: 4 waves x 32
constexpr int WPS = 32;                // pixels per stage
constexpr int T_PITCH = WPS + 1;

template <int NT, bool SOFT, bool VEC>
__global__ __launch_bounds__(256) void ocr_wrw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                      const float* __restrict__ rstats, float scale, int C, int K, long P, int c_tiles,
                                                      int n_split, int B, float* __restrict__ partial) {
    constexpr int KP = NT * 32;
    __shared__ float Xs[WCB * T_PITCH];                        // [channel][pixel]
    __shared__ float Ds[KP * T_PITCH];                         // [class][pixel]
    int blk = blockIdx.x;
    const int split = blk % n_split; blk /= n_split;
    const int ct = blk % c_tiles;
    const int b = blk / c_tiles;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long stages = (P + WPS - 1) / WPS;
    const long s0 = stages * split / n_split, s1 = stages * (split + 1) / n_split;
    const int cb = ct * WCB;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    // loader: thread -> rows tid / 8 + 32 q, four pixels (tid % 8) * 4 ..: eight threads cover the 128 bytes of a row
    const int l_row = tid >> 3, l_px = (tid & 7) * 4;
    float rmx[NT], rinv[NT];
    if (SOFT) {
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int k = min(l_row + 32 * q, K - 1);
            rmx[q] = rstats[(size_t)b * K + k];
            rinv[q] = 1.f / rstats[(size_t)B * K + (size_t)b * K + k];
        }
    }
    float xv[4][4], dv[NT][4];
    auto fetch = [&](long st) {
        const long p0 = st * WPS + l_px;
        const bool full = VEC && p0 + 4 <= P;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = cb + l_row + 32 * q;
            const float* src = x + ((size_t)b * C + min(c, C - 1)) * P;
            if (c < C && full) {
                const float4 t4 = *reinterpret_cast<const float4*>(src + p0);
                xv[q][0] = t4.x; xv[q][1] = t4.y; xv[q][2] = t4.z; xv[q][3] = t4.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) xv[q][j] = (c < C && p0 + j < P) ? src[p0 + j] : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            const int k = l_row + 32 * q;
            const float* src = dy + ((size_t)b * K + min(k, K - 1)) * P;
            if (k < K && full) {
                const float4 t4 = *reinterpret_cast<const float4*>(src + p0);
                dv[q][0] = t4.x; dv[q][1] = t4.y; dv[q][2] = t4.z; dv[q][3] = t4.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) dv[q][j] = (k < K && p0 + j < P) ? src[p0 + j] : 0.f;
            }
            if (SOFT) {
#pragma unroll
                for (int j = 0; j < 4; ++j) dv[q][j] = (k < K && p0 + j < P) ? __expf(scale * dv[q][j] - rmx[q]) * rinv[q] : 0.f;
            }
        }
    };
    if (s0 < s1) fetch(s0);
    for (long st = s0; st < s1; ++st) {
        __syncthreads();                                       // the previous stage has been consumed
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) Xs[(l_row + 32 * q) * T_PITCH + l_px + j] = xv[q][j];
#pragma unroll
        for (int q = 0; q < NT; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) Ds[(l_row + 32 * q) * T_PITCH + l_px + j] = dv[q][j];
        __syncthreads();
        if (st + 1 < s1) fetch(st + 1);
#pragma unroll
        for (int s = 0; s < WPS / 2; ++s) {
            const float a = Xs[(wave * 32 + r) * T_PITCH + 2 * s + h];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float bv = Ds[(t * 32 + r) * T_PITCH + 2 * s + h];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[t], 0, 0, 0);
            }
        }
    }
    float* out = partial + (((size_t)split * B + b) * C + cb + wave * 32) * KP;              // [split][image][channel][class]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int c = d_row(v, h), k = t * 32 + r;
            if (cb + wave * 32 + c < C) out[(size_t)c * KP + k] = k < K ? acc[t][v] : 0.f;
        }
}

// o[b][c][k] = sum over the splits, in order; o has no pad columns
__global__ __launch_bounds__(256) void ocr_wrw_reduce_kernel(const float* __restrict__ partial, int n_split, long rows, int K, int KP,
                                                             float* __restrict__ o) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * K) return;
    const long row = e / K;
    const int k = (int)(e - row * K);
    float s = 0.f;
    for (int sp = 0; sp < n_split; ++sp) s += partial[((size_t)sp * rows + row) * KP + k];
    o[e] = s;
}

// ---- the pixel-axis softmax of the gather: row reductions, one block per (b, k) row ---------------------------------------------------
// the 256 partial values of a block, combined in a fixed order; every thread gets the result
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float* red) {
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();                                           // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
}

// rstats[row] = max_p scale probs, rstats[rows + row] = sum_p exp(scale probs - max)
__global__ __launch_bounds__(256) void ocr_row_stats_kernel(const float* __restrict__ probs, float scale, long P, long rows,
                                                            float* __restrict__ rstats) {
    __shared__ float red[4];
    const long row = blockIdx.x;
    const float* src = probs + (size_t)row * P;
    float mx = -INFINITY;
    for (long p = threadIdx.x; p < P; p += 256) mx = fmaxf(mx, scale * src[p]);
    mx = block_reduce<true>(mx, red);
    float sum = 0.f;
    for (long p = threadIdx.x; p < P; p += 256) sum += __expf(scale * src[p] - mx);
    sum = block_reduce<false>(sum, red);
    if (threadIdx.x == 0) {
        rstats[row] = mx;
        rstats[rows + row] = sum;
    }
}

// in place on g [rows][P]: dprobs = scale s (g - sum_p s g), s recomputed from probs and the row statistics
__global__ __launch_bounds__(256) void ocr_gather_dprobs_kernel(const float* __restrict__ probs, const float* __restrict__ rstats,
                                                                float scale, long P, long rows, float* __restrict__ g) {
    __shared__ float red[4];
    const long row = blockIdx.x;
    const float* src = probs + (size_t)row * P;
    float* gp = g + (size_t)row * P;
    const float mx = rstats[row], inv = 1.f / rstats[rows + row];
    float dot = 0.f;
    for (long p = threadIdx.x; p < P; p += 256) dot += __expf(scale * src[p] - mx) * inv * gp[p];
    dot = block_reduce<false>(dot, red);
    for (long p = threadIdx.x; p < P; p += 256) gp[p] = scale * (__expf(scale * src[p] - mx) * inv) * (gp[p] - dot);
}

int ocr_wrw_splits(int B, int C, int KP, long P) {
    const long stages = (P + WPS - 1) / WPS;
    const long groups = (long)B * ((C + WCB - 1) / WCB);
    // one round of resident blocks: a block is one wave per SIMD, and the registers of the NT accumulator tiles allow 4 / 2 / 1 of them
    // per SIMD on 256 CUs (as cls1x1_wide.hip)
    const long resident = 256 * (KP <= 96 ? 4 : KP <= 224 ? 2 : 1);
    long n = resident / groups;
    if (n > stages) n = stages;
    if (n > 64) n = 64;
    return (int)(n < 1 ? 1 : n);
}

// the KP rule is kernels.ocr_kp of contrastiveseg_amd/kernels.py (cls1x1_wide_kp(K), at least 64): keep the two in step
bool ocr_shape_ok(int B, int C, int K, int KP, long P) {
    return B > 0 && C > 0 && K >= 2 && K <= 256 && KP == (K <= 64 ? 64 : (K + 31) / 32 * 32) && P > 0 && (long)B * C * P < (1L << 40) &&
           (long)B * K * P < (1L << 40) && (long)B * ((P + PXB - 1) / PXB) < 2147483647L / 16 && (long)B * K < 2147483647L;
}

#define OCR_DISPATCH(NTV, CALL)                                                                                                       \
    switch (NTV) {                                                                                                                    \
        case 2: CALL(2); break;                                                                                                       \
        case 3: CALL(3); break;                                                                                                       \
        case 4: CALL(4); break;                                                                                                       \
        case 5: CALL(5); break;                                                                                                       \
        case 6: CALL(6); break;                                                                                                       \
        case 7: CALL(7); break;                                                                                                       \
        default: CALL(8); break;                                                                                                      \
    }

template <int MODE>
int launch_pixel(const char* who, const float* x, const float* w, const float* aux, float scale, int B, int C, int K, int KP, long P,
                 float* out, float* stats, hipStream_t stream) {
    const int tiles = (int)((P + PXB - 1) / PXB);
#define OCR_PIX(NTV)                                                                                                                  \
    hipLaunchKernelGGL((ocr_pixel_kernel<NTV, MODE>), dim3((unsigned)(B * tiles)), dim3(256), 0, stream, x, w, aux, scale, C, K, P,   \
                       tiles, out, stats)
    OCR_DISPATCH(KP / 32, OCR_PIX)
#undef OCR_PIX
    CSEG_CHECK_LAUNCH(who);
    return 1;
}

template <bool SOFT>
int launch_bwd(const char* who, const float* dy, const float* w, const float* rstats, float scale, int B, int C, int K, int KP, long P,
               float* dx, hipStream_t stream) {
    const int tiles = (int)((P + PXB - 1) / PXB), c_tiles = (C + CC - 1) / CC;
    int parts = 1;                                             // channel parts: enough blocks for the chip (each re-reads its pixels' d)
    while (parts < 16 && (long)B * tiles * parts < 1024 && c_tiles / (parts * 2) >= 2) parts *= 2;
#define OCR_BWD(NTV)                                                                                                                  \
    hipLaunchKernelGGL((ocr_bwd_kernel<NTV, SOFT>), dim3((unsigned)(B * tiles), parts), dim3(256), 0, stream, dy, w, rstats, scale, B, \
                       C, K, P, tiles, dx)
    OCR_DISPATCH(KP / 32, OCR_BWD)
#undef OCR_BWD
    CSEG_CHECK_LAUNCH(who);
    return 1;
}

// o [B][C][K] = sum_p x[b][c][p] d[b][k][p]; ws: ocr_wrw_splits(...) * B * C * KP floats
template <bool SOFT>
int launch_wrw(const char* who, const float* x, const float* dy, const float* rstats, float scale, int B, int C, int K, int KP, long P,
               float* ws, float* o, hipStream_t stream) {
    const int n_split = ocr_wrw_splits(B, C, KP, P), c_tiles = (C + WCB - 1) / WCB;
    const long blocks = (long)B * c_tiles * n_split;
    const bool vec = P % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy)) & 15) == 0;
#define OCR_WRW(NTV)                                                                                                                  \
    do {                                                                                                                              \
        if (vec)                                                                                                                      \
            hipLaunchKernelGGL((ocr_wrw_kernel<NTV, SOFT, true>), dim3((unsigned)blocks), dim3(256), 0, stream, x, dy, rstats, scale, \
                               C, K, P, c_tiles, n_split, B, ws);                                                                     \
        else                                                                                                                          \
            hipLaunchKernelGGL((ocr_wrw_kernel<NTV, SOFT, false>), dim3((unsigned)blocks), dim3(256), 0, stream, x, dy, rstats,       \
                               scale, C, K, P, c_tiles, n_split, B, ws);                                                              \
    } while (0)
    OCR_DISPATCH(KP / 32, OCR_WRW)
#undef OCR_WRW
    CSEG_CHECK_LAUNCH(who);
    const long rows = (long)B * C;
    hipLaunchKernelGGL(ocr_wrw_reduce_kernel, dim3((unsigned)((rows * K + 255) / 256)), dim3(256), 0, stream, ws, n_split, rows, K, KP, o);
    CSEG_CHECK_LAUNCH(who);
    return 1;
}

size_t wrw_ws(int B, int C, int KP, long P) { return (size_t)ocr_wrw_splits(B, C, KP, P) * B * C * KP; }

}  // namespace

#define OCR_SHAPE(name)                                                                                                               \
    CSEG_REQUIRE(ocr_shape_ok(B, C, K, KP, P),                                                                                        \
                 name ": unsupported shape B=%d C=%d K=%d KP=%d P=%ld (2 <= K <= 256, KP = K rounded up to 32, at least 64)", B, C, K, \
                 KP, P)

extern "C" size_t cseg_ocr_gather_ws_floats(int B, int C, int K, int KP, long P) {
    if (!ocr_shape_ok(B, C, K, KP, P)) return 0;
    return wrw_ws(B, C, KP, P) + 2 * (size_t)B * K;
}

extern "C" int cseg_ocr_gather_fwd(const float* probs, const float* feats, float scale, int B, int C, int K, int KP, long P, float* ws,
                                   float* rstats, float* ctx, cseg_stream_t stream_) {
    CSEG_REQUIRE(probs && feats && ws && ctx, "ocr_gather_fwd: null pointer");
    OCR_SHAPE("ocr_gather_fwd");
    hipStream_t stream = (hipStream_t)stream_;
    if (!rstats) rstats = ws + wrw_ws(B, C, KP, P);            // no backward to come: the statistics live in the workspace
    const long rows = (long)B * K;
    hipLaunchKernelGGL(ocr_row_stats_kernel, dim3((unsigned)rows), dim3(256), 0, stream, probs, scale, P, rows, rstats);
    CSEG_CHECK_LAUNCH("ocr_gather_fwd");
    return launch_wrw<true>("ocr_gather_fwd", feats, probs, rstats, scale, B, C, K, KP, P, ws, ctx, stream);
}

extern "C" int cseg_ocr_gather_bwd(const float* probs, const float* feats, const float* rstats, const float* dctx, float scale, int B,
                                   int C, int K, int KP, long P, float* dprobs, float* dfeats, cseg_stream_t stream_) {
    CSEG_REQUIRE(probs && feats && rstats && dctx && (dprobs || dfeats), "ocr_gather_bwd: null pointer");
    OCR_SHAPE("ocr_gather_bwd");
    hipStream_t stream = (hipStream_t)stream_;
    if (dprobs) {
        if (!launch_pixel<M_PLAIN>("ocr_gather_bwd", feats, dctx, nullptr, scale, B, C, K, KP, P, dprobs, nullptr, stream)) return 0;
        const long rows = (long)B * K;
        hipLaunchKernelGGL(ocr_gather_dprobs_kernel, dim3((unsigned)rows), dim3(256), 0, stream, probs, rstats, scale, P, rows, dprobs);
        CSEG_CHECK_LAUNCH("ocr_gather_bwd");
    }
    if (dfeats) return launch_bwd<true>("ocr_gather_bwd", probs, dctx, rstats, scale, B, C, K, KP, P, dfeats, stream);
    return 1;
}

extern "C" int cseg_ocr_attn_fwd(const float* q, const float* key, const float* value, float scale, int B, int C, int K, int KP, long P,
                                 float* out, float* stats, cseg_stream_t stream_) {
    CSEG_REQUIRE(q && key && value && out, "ocr_attn_fwd: null pointer");
    OCR_SHAPE("ocr_attn_fwd");
    hipStream_t stream = (hipStream_t)stream_;
    if (stats) return launch_pixel<M_ATTN_STATS>("ocr_attn_fwd", q, key, value, scale, B, C, K, KP, P, out, stats, stream);
    return launch_pixel<M_ATTN>("ocr_attn_fwd", q, key, value, scale, B, C, K, KP, P, out, nullptr, stream);
}

extern "C" size_t cseg_ocr_attn_bwd_ws_floats(int B, int C, int K, int KP, long P) {
    if (!ocr_shape_ok(B, C, K, KP, P)) return 0;
    return 2 * (size_t)B * K * P + wrw_ws(B, C, KP, P);
}

extern "C" int cseg_ocr_attn_bwd(const float* q, const float* key, const float* value, const float* stats, const float* dout,
                                 float scale, int B, int C, int K, int KP, long P, float* ws, float* dq, float* dkey, float* dvalue,
                                 cseg_stream_t stream_) {
    CSEG_REQUIRE(q && key && value && stats && dout && ws && dq && dkey && dvalue, "ocr_attn_bwd: null pointer");
    OCR_SHAPE("ocr_attn_bwd");
    hipStream_t stream = (hipStream_t)stream_;
    float* a = ws;                                             // [B][K][P], written once, read by the next kernel and by dvalue
    float* dl = ws + (size_t)B * K * P;                        // [B][K][P], written once, read by dq and dkey
    float* part = dl + (size_t)B * K * P;
    if (!launch_pixel<M_PROB>("ocr_attn_bwd", q, key, stats, scale, B, C, K, KP, P, a, nullptr, stream)) return 0;
    if (!launch_pixel<M_DLOGIT>("ocr_attn_bwd", dout, value, a, scale, B, C, K, KP, P, dl, nullptr, stream)) return 0;
    if (!launch_bwd<false>("ocr_attn_bwd", dl, key, nullptr, scale, B, C, K, KP, P, dq, stream)) return 0;
    if (!launch_wrw<false>("ocr_attn_bwd", q, dl, nullptr, scale, B, C, K, KP, P, part, dkey, stream)) return 0;
    return launch_wrw<false>("ocr_attn_bwd", dout, a, nullptr, scale, B, C, K, KP, P, part, dvalue, stream);
}
