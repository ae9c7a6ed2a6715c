// Lovasz-softmax segmentation term: lovasz_softmax_flat(*flatten_probas(softmax(F.interpolate(seg)), target, ignore), only_present=True)
// of the reference (lib/loss/lovasz_loss.py:216-267, used by FSCELOVASZLoss, lib/loss/loss_helper.py:77-124) on the coarse logits. The
// reference builds the [B,K,H,W] softmax and a permuted copy, calls nonzero, asks the host once per class whether the class is present
// and runs one torch.sort per class; here the route is a segmented LSD radix sort and a segmented scan, and nothing in it depends on
// data on the host. P = B * H * W label pixels; a pixel is valid when 0 <= label < K; the sort segment of a class is all P pixels:
// invalid ones are not compacted away (that needs a data-dependent size), they carry a key that sorts after every valid pixel.
//
// Sort key (u32): bit 0 = fg (label == class), bits 1..30 = 0x3F800000 - bits(e) for a valid pixel, 0x3F800001 for an invalid one, where
// e = |fg - p| lies in [0, 1], so its fp32 bits lie in [0, 0x3F800000]. Ascending order of bits 1..30, stable = descending e, ascending
// flat pixel index among equal e: the order of torch.sort(stable=True, descending=True). fg takes no part in the order.
//
// Launches (no block ever waits for another one: every cross-tile dependency is a launch boundary; no floating-point atomics):
//   lov_errors_kernel   thread = one label pixel: interpolates the K logits (taps: DESIGN.md section 26), softmax (max, then sum; logits in float64), keys of the
//                       classes [k0, k0 + kn); optionally e / fg planes and the exact counts (integer atomics).
//   lov_pack_kernel     e / fg planes (optionally gathered through a permutation) -> keys: the stage entry points of the tests.
//   per radix pass (8 passes of 4 bits over bits 1..32):
//     lov_hist_kernel     block = one tile of 2048 keys of one class -> digit counts hist[class][digit][tile]
//     lov_scan_kernel     block = one class: exclusive scan over [digit][tile]
//     lov_scatter_kernel  block = one tile: stable rank of every key among the keys of its digit in the tile (prefix sums over
//                         [digit][thread], thread-blocked arrangement; never the return value of an atomic) + the scanned base
//   lov_fgsum_kernel    fg sums per tile of the sorted order; lov_scan_kernel turns them into tile offsets and the class total G
//   lov_apply_kernel    inclusive fg count c_r per sorted position r -> J_r = 1 - (G - c_r) / (G + (r + 1 - c_r)) from the exact
//                       integers in float64, g_r = J_r - J_(r-1), per-tile sum of e_(r) g_r in float64 (fixed order); g_r goes with
//                       the sign of d e / d p (-1 for fg, +1 otherwise, 0 where e == 0) to G_buf [K,P] f32 at the payload index.
//   lov_finish_kernel   one block: loss_c, the number of present classes, the term.
//   lov_pix_kernel      backward, thread = one label pixel: softmax statistics and D = sum_k p_k G_k
//   lov_bwd_kernel      backward, thread = one coarse logit: the gather adjoint (bl_gather_adjoint) of
//                       d z_c = p_c (G_c - D), times d_loss / n_present.
#include "cseg_taps.h"

namespace {

constexpr int LV_THREADS = 256;
constexpr int LV_ITEMS = 8;                         // consecutive keys per thread (<= 15: 4-bit local counters)
constexpr int LV_TILE = LV_THREADS * LV_ITEMS;      // 2048 keys
constexpr int LV_BINS = 16;                         // 4-bit digits
constexpr int LV_PASSES = 8;                        // bits 1 .. 32 (bit 31 is always 0)
constexpr int LV_CNT = LV_BINS * LV_THREADS + LV_BINS * LV_THREADS / 16;   // [digit][thread] counters, one pad word per 16
constexpr unsigned LV_ONE = 0x3F800000u;            // bits of 1.0f
constexpr unsigned LV_VOID = LV_ONE + 1u;           // sort field of an invalid pixel: after every valid one

__device__ __forceinline__ int lv_idx(int i) { return i + (i >> 4); }

struct LvDims : UpDims {
    int P;
};

__device__ __forceinline__ unsigned lv_pack(float e, unsigned fg) {
    if (!(e >= 0.f)) return LV_VOID << 1;
    const unsigned bits = min(__builtin_bit_cast(unsigned, fabsf(e)), LV_ONE);
    return ((LV_ONE - bits) << 1) | (fg & 1u);
}

__device__ __forceinline__ float lv_error(unsigned key) {
    const unsigned field = key >> 1;
    return field > LV_ONE ? -1.f : __builtin_bit_cast(float, LV_ONE - field);
}

struct LvTap {
    int y0, y1, x0, x1;
    float ly1, lx1;
};

// One interpolated logit in float64 from the fp32 taps and the fp32 weights of cseg_taps.h (torch's own index arithmetic, so the
// weights are torch's): the rounding of an fp32 interpolation is one ulp of the logit, which at |x| ~ 100 is 1e-5 of a probability --
// more than the reference's own fp32 deviation on some inputs. Only differences and explicit fma: nothing is left for the compiler to
// contract one way in one inlined copy and another way in the next (the passes below rely on equal inputs giving equal values).
__device__ __forceinline__ double lv_logit(const float* __restrict__ plane, int w, const LvTap& t) {
    const double v00 = plane[(size_t)t.y0 * w + t.x0], v10 = plane[(size_t)t.y1 * w + t.x0];
    const double v01 = plane[(size_t)t.y0 * w + t.x1], v11 = plane[(size_t)t.y1 * w + t.x1];
    const double ly1 = t.ly1;
    const double r0 = fma(ly1, v10 - v00, v00);
    const double r1 = fma(ly1, v11 - v01, v01);
    return fma((double)t.lx1, r1 - r0, r0);
}

// exp(x - m) of the softmax: the difference in float64, the exponential in fp32
__device__ __forceinline__ float lv_exp(double x, float m) { return expf((float)(x - (double)m)); }

// softmax statistics of one label pixel as torch computes them: the maximum first (rounded up to fp32: any shift serves, as long as the
// numerator uses the same one, and this one keeps every exponent <= 0), then the sum of exp(x - max) in fp32
__device__ __forceinline__ void lv_softmax_stats(const float* __restrict__ img, int K, int hw, int w, const LvTap& t, float& m, float& s) {
    double mx = lv_logit(img, w, t);
    for (int k = 1; k < K; ++k) mx = fmax(mx, lv_logit(img + (size_t)k * hw, w, t));
    m = (float)mx;
    if ((double)m < mx) m = nextafterf(m, INFINITY);
    s = 0.f;
    for (int k = 0; k < K; ++k) s += lv_exp(lv_logit(img + (size_t)k * hw, w, t), m);
}

__device__ __forceinline__ void lv_pixel(const LvDims& d, int i, int& b, LvTap& t) {
    const int X = i % d.W;
    const int r = i / d.W;
    const int Y = r % d.H;
    b = r / d.H;
    bl_tap(d.sy, d.h, Y, t.y0, t.y1, t.ly1);
    bl_tap(d.sx, d.w, X, t.x0, t.x1, t.lx1);
}

__global__ __launch_bounds__(256) void lov_zero_kernel(int* __restrict__ p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// ---------------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lov_errors_kernel(const float* __restrict__ seg, const int64_t* __restrict__ target, LvDims d,
                                                         int ignore_label, int k0, int kn, unsigned* __restrict__ keys,
                                                         float* __restrict__ e_out, uint8_t* __restrict__ fg_out,
                                                         int* __restrict__ counts, int* __restrict__ status) {
    __shared__ int s_cnt[258];                       // per class, valid pixels, bad labels
    const int tid = threadIdx.x;
    for (int j = tid; j < 258; j += 256) s_cnt[j] = 0;
    __syncthreads();
    const long gi = (long)blockIdx.x * 256 + tid;
    if (gi < d.P) {
        const int i = (int)gi;
        const int64_t t64 = target[i];
        const bool valid = t64 >= 0 && t64 < d.K;
        if (valid) {
            int b;
            LvTap t;
            lv_pixel(d, i, b, t);
            const int hw = d.h * d.w;
            const float* img = seg + (size_t)b * d.K * hw;
            float m, s;
            lv_softmax_stats(img, d.K, hw, d.w, t, m, s);
            for (int c = 0; c < kn; ++c) {
                const int k = k0 + c;
                const float p = fminf(lv_exp(lv_logit(img + (size_t)k * hw, d.w, t), m) / s, 1.f);
                const unsigned fg = t64 == k ? 1u : 0u;
                const float e = fabsf((fg ? 1.f : 0.f) - p);
                if (keys) keys[(size_t)c * d.P + i] = lv_pack(e, fg);
                if (e_out) e_out[(size_t)k * d.P + i] = e;
                if (fg_out) fg_out[(size_t)k * d.P + i] = (uint8_t)fg;
            }
            atomicAdd(&s_cnt[(int)t64], 1);
            atomicAdd(&s_cnt[256], 1);
        } else {
            for (int c = 0; c < kn; ++c) {
                if (keys) keys[(size_t)c * d.P + i] = LV_VOID << 1;
                if (e_out) e_out[(size_t)(k0 + c) * d.P + i] = -1.f;
                if (fg_out) fg_out[(size_t)(k0 + c) * d.P + i] = 0;
            }
            if (t64 != ignore_label) atomicAdd(&s_cnt[257], 1);
        }
    }
    __syncthreads();
    if (counts) {
        for (int j = tid; j < d.K; j += 256)
            if (s_cnt[j]) atomicAdd(&counts[j], s_cnt[j]);
        if (tid == 0 && s_cnt[256]) atomicAdd(&counts[d.K], s_cnt[256]);
        if (tid == 0 && s_cnt[257]) atomicAdd(&counts[d.K + 1], s_cnt[257]);
    }
    if (status && tid == 0 && s_cnt[257]) atomicAdd(&status[1], s_cnt[257]);
}

// keys[c][r] = pack(e[c][j], fg[c][j]) with j = perm[c][r], or j = r without a permutation
__global__ __launch_bounds__(256) void lov_pack_kernel(const float* __restrict__ e, const uint8_t* __restrict__ fg,
                                                       const int* __restrict__ perm, int P, unsigned* __restrict__ keys) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const size_t row = (size_t)blockIdx.y * P;
    if (r >= P) return;
    int j = (int)r;
    if (perm) {
        j = perm[row + r];
        if ((unsigned)j >= (unsigned)P) { keys[row + r] = LV_VOID << 1; return; }
    }
    keys[row + r] = lv_pack(e[row + j], fg[row + j] ? 1u : 0u);
}

// ---------------------------------------------------------------------------------------------------------
// order: one 4-bit pass of a stable LSD radix sort per class segment
// ---------------------------------------------------------------------------------------------------------
// The keys of a tile in thread-blocked arrangement: thread t holds the keys LV_ITEMS * t .. + LV_ITEMS - 1 of the tile. `packed` holds
// the thread's count per digit in 4-bit fields. After the call s_cnt[lv_idx(digit * 256 + thread)] is the number of keys of the tile
// that sort before the first key of that digit in that thread: smaller digits, and the same digit in earlier threads.
__device__ __forceinline__ void lv_tile_scan(unsigned long long packed, int* s_cnt, int* s_wave) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int dg = 0; dg < LV_BINS; ++dg) s_cnt[lv_idx(dg * LV_THREADS + tid)] = (int)((packed >> (4 * dg)) & 15ull);
    __syncthreads();
    int v[16], sum = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        v[j] = s_cnt[lv_idx(16 * tid + j)];
        sum += v[j];
    }
    const int incl = wave_incl_scan_i(sum, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int wv = 0; wv < wave; ++wv) run += s_wave[wv];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        s_cnt[lv_idx(16 * tid + j)] = run;
        run += v[j];
    }
    __syncthreads();
}

__device__ __forceinline__ unsigned long long lv_load_tile(const unsigned* __restrict__ seg_keys, int P, long first, int shift,
                                                           unsigned key[LV_ITEMS], int rank[LV_ITEMS]) {
    unsigned long long packed = 0ull;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        key[j] = 0u;
        rank[j] = 0;
        if (first + j < P) {
            key[j] = seg_keys[first + j];
            const int dg = (int)((key[j] >> shift) & 15u);
            rank[j] = (int)((packed >> (4 * dg)) & 15ull);
            packed += 1ull << (4 * dg);
        }
    }
    return packed;
}

// grid = (T, classes): hist[(class * 16 + digit) * T + tile]; every word is written
__global__ __launch_bounds__(LV_THREADS) void lov_hist_kernel(const unsigned* __restrict__ keys, int P, int T, int shift,
                                                              int* __restrict__ hist) {
    __shared__ int s_cnt[LV_CNT];
    __shared__ int s_wave[4];
    const int tile = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const long first = (long)tile * LV_TILE + tid * LV_ITEMS;
    unsigned key[LV_ITEMS];
    int rank[LV_ITEMS];
    const unsigned long long packed = lv_load_tile(keys + (size_t)c * P, P, first, shift, key, rank);
    lv_tile_scan(packed, s_cnt, s_wave);
    if (tid < LV_BINS) {
        const int n_tile = min(LV_TILE, P - tile * LV_TILE);
        const int lo = s_cnt[lv_idx(tid * LV_THREADS)];
        const int hi = tid + 1 < LV_BINS ? s_cnt[lv_idx((tid + 1) * LV_THREADS)] : n_tile;
        hist[((size_t)c * LV_BINS + tid) * T + tile] = hi - lo;
    }
}

// in-place exclusive scan of n integers per block (one class); the total goes to totals[block] when asked for
__global__ __launch_bounds__(1024) void lov_scan_kernel(int* __restrict__ data, int n, int* __restrict__ totals) {
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* d = data + (size_t)blockIdx.x * n;
    const int per = (n + 1023) / 1024;
    const int lo = (int)min((long)n, (long)tid * per), hi = (int)min((long)n, (long)lo + per);
    int sum = 0;
    for (int j = lo; j < hi; ++j) sum += d[j];
    const int incl = wave_incl_scan_i(sum, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int wv = 0; wv < wave; ++wv) run += s_wave[wv];
    for (int j = lo; j < hi; ++j) {
        const int v = d[j];
        d[j] = run;
        run += v;
    }
    if (totals && tid == 1023) totals[blockIdx.x] = run;
}

// grid = (T, classes); base = the scanned hist. pay_in == nullptr: the payload is the position itself (first pass)
__global__ __launch_bounds__(LV_THREADS) void lov_scatter_kernel(const unsigned* __restrict__ keys_in, const int* __restrict__ pay_in,
                                                                 int P, int T, int shift, const int* __restrict__ base,
                                                                 unsigned* __restrict__ keys_out, int* __restrict__ pay_out) {
    __shared__ int s_cnt[LV_CNT];
    __shared__ int s_wave[4];
    __shared__ int s_off[LV_BINS];
    const int tile = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const size_t row = (size_t)c * P;
    const long first = (long)tile * LV_TILE + tid * LV_ITEMS;
    unsigned key[LV_ITEMS];
    int rank[LV_ITEMS];
    const unsigned long long packed = lv_load_tile(keys_in + row, P, first, shift, key, rank);
    lv_tile_scan(packed, s_cnt, s_wave);
    if (tid < LV_BINS) s_off[tid] = base[((size_t)c * LV_BINS + tid) * T + tile] - s_cnt[lv_idx(tid * LV_THREADS)];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        if (first + j < P) {
            const int dg = (int)((key[j] >> shift) & 15u);
            const int dst = s_off[dg] + s_cnt[lv_idx(dg * LV_THREADS + tid)] + rank[j];
            if ((unsigned)dst < (unsigned)P) {          // (always: the counts come from these very keys)
                keys_out[row + dst] = key[j];
                pay_out[row + dst] = pay_in ? pay_in[row + first + j] : (int)(first + j);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// grad: segmented inclusive scan of fg along the sorted order, Jaccard differences in float64
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LV_THREADS) void lov_fgsum_kernel(const unsigned* __restrict__ keys, int P, int T, int* __restrict__ tsum) {
    __shared__ int s_wave[4];
    const int tile = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const unsigned* k = keys + (size_t)c * P;
    const long first = (long)tile * LV_TILE + tid * LV_ITEMS;
    int sum = 0;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j)
        if (first + j < P) sum += (int)(k[first + j] & 1u);
    sum = wave_sum_i(sum);
    if ((tid & 63) == 0) s_wave[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) tsum[(size_t)c * T + tile] = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}

__global__ __launch_bounds__(LV_THREADS) void lov_apply_kernel(const unsigned* __restrict__ keys, const int* __restrict__ pay, int P, int T,
                                                               const int* __restrict__ toff, const int* __restrict__ gtot,
                                                               double* __restrict__ g_sorted, float* __restrict__ gbuf,
                                                               double* __restrict__ partial) {
    __shared__ int s_wave[4];
    __shared__ double s_red[4];
    const int tile = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)c * P;
    const long first = (long)tile * LV_TILE + tid * LV_ITEMS;
    unsigned key[LV_ITEMS];
    int sum = 0;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        key[j] = first + j < P ? keys[row + first + j] : (LV_VOID << 1);
        sum += (int)(key[j] & 1u);
    }
    const int incl = wave_incl_scan_i(sum, lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int cf = toff[(size_t)c * T + tile] + incl - sum;          // fg among the positions before this thread's
    for (int wv = 0; wv < wave; ++wv) cf += s_wave[wv];
    const int G = gtot[c];
    const double Gd = (double)G;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        if (first + j >= P) continue;
        const int r = (int)(first + j);
        const int fg = (int)(key[j] & 1u);
        const int cprev = cf;
        cf += fg;
        const float e = lv_error(key[j]);
        double g = 0.0;
        if (G > 0 && e >= 0.f) {
            const double jr = 1.0 - (Gd - (double)cf) / (Gd + (double)(r + 1 - cf));
            const double jp = r > 0 ? 1.0 - (Gd - (double)cprev) / (Gd + (double)(r - cprev)) : 0.0;
            g = jr - jp;
            acc += (double)e * g;
        }
        if (g_sorted) g_sorted[row + r] = g;
        if (gbuf) {
            const int px = pay[row + r];
            if ((unsigned)px < (unsigned)P) gbuf[row + px] = e > 0.f ? (float)(fg ? -g : g) : 0.f;
        }
    }
    acc = wave_sum_d(acc);
    if (lane == 0) s_red[wave] = acc;
    __syncthreads();
    if (tid == 0) partial[(size_t)c * T + tile] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// one block: loss_c[K] (0 for an absent class), outd = {term, present classes}, out = (float)term
__global__ __launch_bounds__(256) void lov_finish_kernel(const double* __restrict__ partial, const int* __restrict__ gtot, int K, int T,
                                                         double* __restrict__ loss_c, double* __restrict__ outd, float* __restrict__ out) {
    __shared__ double s_loss[256];
    __shared__ int s_present[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    int present = 0;
    if (tid < K) {
        present = gtot[tid] > 0 ? 1 : 0;
        if (present)
            for (int t = 0; t < T; ++t) s += partial[(size_t)tid * T + t];
        if (loss_c) loss_c[tid] = s;
    }
    s_loss[tid] = s;
    s_present[tid] = present;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        int n = 0;
        for (int k = 0; k < K; ++k) {
            total += s_loss[k];
            n += s_present[k];
        }
        const double term = n > 0 ? total / (double)n : 0.0;
        outd[0] = term;
        outd[1] = (double)n;
        out[0] = (float)term;
    }
}

// ---------------------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------------------
// stats [3][P]: max, sum of exp (0 for an invalid pixel: it has no gradient), D = sum_k p_k G_k
__global__ __launch_bounds__(256) void lov_pix_kernel(const float* __restrict__ seg, const int64_t* __restrict__ target, LvDims d,
                                                      const float* __restrict__ gbuf, float* __restrict__ stats) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= d.P) return;
    const int i = (int)gi;
    const int64_t t64 = target[i];
    float m = 0.f, s = 0.f, D = 0.f;
    if (t64 >= 0 && t64 < d.K) {
        int b;
        LvTap t;
        lv_pixel(d, i, b, t);
        const int hw = d.h * d.w;
        const float* img = seg + (size_t)b * d.K * hw;
        lv_softmax_stats(img, d.K, hw, d.w, t, m, s);
        for (int k = 0; k < d.K; ++k) D += fminf(lv_exp(lv_logit(img + (size_t)k * hw, d.w, t), m) / s, 1.f) * gbuf[(size_t)k * d.P + i];
    }
    stats[i] = m;
    stats[(size_t)d.P + i] = s;
    stats[2 * (size_t)d.P + i] = D;
}

// grid = (h * w / 256, K, B)
__global__ __launch_bounds__(256) void lov_bwd_kernel(const float* __restrict__ seg, const float* __restrict__ gbuf,
                                                      const float* __restrict__ stats, LvDims d, const double* __restrict__ outd,
                                                      const float* __restrict__ d_loss, float* __restrict__ d_seg) {
    const int k = blockIdx.y, b = blockIdx.z;
    const int cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= d.h * d.w) return;
    const int ys = cell / d.w, xs = cell - ys * d.w;
    const float scale = outd[1] > 0.0 ? (float)((double)d_loss[0] / outd[1]) : 0.f;
    const float* plane = seg + ((size_t)b * d.K + k) * d.h * d.w;
    const float* grow = gbuf + (size_t)k * d.P;
    const float acc = bl_gather_adjoint(d.sy, d.sx, d.h, d.w, d.H, d.W, ys, xs,
                                        [&](int Y, int X, int y0, int y1, float ly1, int x0, int x1, float lx1, float& v) {
        const size_t i = ((size_t)b * d.H + Y) * d.W + X;
        const float s = stats[(size_t)d.P + i];
        if (!(s > 0.f)) return false;                              // invalid pixel
        const float p = fminf(lv_exp(lv_logit(plane, d.w, LvTap{y0, y1, x0, x1, ly1, lx1}), stats[i]) / s, 1.f);
        v = p * (grow[i] - stats[2 * (size_t)d.P + i]);
        return true;
    });
    d_seg[(((size_t)b * d.K + k) * d.h + ys) * d.w + xs] = acc * scale;
}

int lov_dims(LvDims* d, int B, int K, int h, int w, int H, int W) {
    if (!up_dims("lovasz", d, B, K, h, w, H, W)) return 0;
    CSEG_REQUIRE(K <= 256, "lovasz: %d classes (at most 256 are implemented)", K);
    CSEG_REQUIRE((long)B * H * W < 2147483648L, "lovasz: %ld label pixels (P = B * H * W must be below 2^31)", (long)B * H * W);
    CSEG_REQUIRE((long)B * K * h * w < 2147483647L, "lovasz: tensor too large");
    d->P = B * H * W;
    return 1;
}

int lov_segments(int n, int P) {
    CSEG_REQUIRE(n > 0 && n <= 256, "lovasz: %d class segments (1 .. 256)", n);
    CSEG_REQUIRE(P > 0, "lovasz: empty segments");
    return 1;
}

}  // namespace

extern "C" int cseg_lovasz_tiles(long P) {
    if (P <= 0 || P >= 2147483648L) return 0;
    return (int)((P + LV_TILE - 1) / LV_TILE);
}

extern "C" int cseg_lovasz_errors(const float* seg, const int64_t* target, int ignore_label, int B, int K, int h, int w, int H, int W,
                                  int k0, int kn, uint32_t* keys, float* e, uint8_t* fg, int32_t* counts, int32_t* status,
                                  cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LvDims d;
    if (!lov_dims(&d, B, K, h, w, H, W)) return 0;
    CSEG_REQUIRE(k0 >= 0 && kn > 0 && k0 + kn <= K, "lovasz_errors: classes [%d, %d) of %d", k0, k0 + kn, K);
    if (counts) {
        hipLaunchKernelGGL(lov_zero_kernel, dim3((K + 2 + 255) / 256), dim3(256), 0, stream, counts, K + 2);
        CSEG_CHECK_LAUNCH("lov_zero_kernel");
    }
    hipLaunchKernelGGL(lov_errors_kernel, dim3((unsigned)(((long)d.P + 255) / 256)), dim3(256), 0, stream, seg, target, d, ignore_label, k0,
                       kn, keys, e, fg, counts, status);
    CSEG_CHECK_LAUNCH("lov_errors_kernel");
    return 1;
}

extern "C" int cseg_lovasz_pack(const float* e, const uint8_t* fg, const int32_t* perm, int n, int P, uint32_t* keys,
                                cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!lov_segments(n, P)) return 0;
    hipLaunchKernelGGL(lov_pack_kernel, dim3((unsigned)(((long)P + 255) / 256), n), dim3(256), 0, stream, e, fg, perm, P, keys);
    CSEG_CHECK_LAUNCH("lov_pack_kernel");
    return 1;
}

extern "C" int cseg_lovasz_order(uint32_t* keys_a, int32_t* pay_a, uint32_t* keys_b, int32_t* pay_b, int32_t* hist, int n, int P,
                                 cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!lov_segments(n, P)) return 0;
    const int T = cseg_lovasz_tiles(P);
    for (int pass = 0; pass < LV_PASSES; ++pass) {
        const int shift = 1 + 4 * pass;
        const unsigned* kin = (pass & 1) ? keys_b : keys_a;
        const int* pin = pass == 0 ? nullptr : ((pass & 1) ? pay_b : pay_a);
        unsigned* kout = (pass & 1) ? keys_a : keys_b;
        int* pout = (pass & 1) ? pay_a : pay_b;
        hipLaunchKernelGGL(lov_hist_kernel, dim3(T, n), dim3(LV_THREADS), 0, stream, kin, P, T, shift, hist);
        CSEG_CHECK_LAUNCH("lov_hist_kernel");
        hipLaunchKernelGGL(lov_scan_kernel, dim3(n), dim3(1024), 0, stream, hist, LV_BINS * T, (int*)nullptr);
        CSEG_CHECK_LAUNCH("lov_scan_kernel");
        hipLaunchKernelGGL(lov_scatter_kernel, dim3(T, n), dim3(LV_THREADS), 0, stream, kin, pin, P, T, shift, (const int*)hist, kout, pout);
        CSEG_CHECK_LAUNCH("lov_scatter_kernel");
    }
    return 1;                                          // an even number of passes: the result is in keys_a / pay_a
}

extern "C" int cseg_lovasz_grad(const uint32_t* keys, const int32_t* pay, int n, int P, int32_t* toff, int32_t* gtot, double* g_sorted,
                                float* gbuf, double* partial, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!lov_segments(n, P)) return 0;
    CSEG_REQUIRE(gbuf == nullptr || pay != nullptr, "lovasz_grad: the scatter needs the payload");
    const int T = cseg_lovasz_tiles(P);
    hipLaunchKernelGGL(lov_fgsum_kernel, dim3(T, n), dim3(LV_THREADS), 0, stream, keys, P, T, toff);
    CSEG_CHECK_LAUNCH("lov_fgsum_kernel");
    hipLaunchKernelGGL(lov_scan_kernel, dim3(n), dim3(1024), 0, stream, toff, T, gtot);
    CSEG_CHECK_LAUNCH("lov_scan_kernel");
    hipLaunchKernelGGL(lov_apply_kernel, dim3(T, n), dim3(LV_THREADS), 0, stream, keys, pay, P, T, (const int*)toff, (const int*)gtot,
                       g_sorted, gbuf, partial);
    CSEG_CHECK_LAUNCH("lov_apply_kernel");
    return 1;
}

extern "C" int cseg_lovasz_finish(const double* partial, const int32_t* gtot, int K, int P, double* loss_c, double* outd, float* out,
                                  cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!lov_segments(K, P)) return 0;
    hipLaunchKernelGGL(lov_finish_kernel, dim3(1), dim3(256), 0, stream, partial, gtot, K, cseg_lovasz_tiles(P), loss_c, outd, out);
    CSEG_CHECK_LAUNCH("lov_finish_kernel");
    return 1;
}

extern "C" int cseg_lovasz_bwd(const float* seg, const int64_t* target, const float* gbuf, const double* outd, const float* d_loss, int B,
                               int K, int h, int w, int H, int W, float* stats, float* d_seg, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    LvDims d;
    if (!lov_dims(&d, B, K, h, w, H, W)) return 0;
    CSEG_REQUIRE(B <= 65535, "lovasz_bwd: %d images exceed the grid", B);
    hipLaunchKernelGGL(lov_pix_kernel, dim3((unsigned)(((long)d.P + 255) / 256)), dim3(256), 0, stream, seg, target, d, gbuf, stats);
    CSEG_CHECK_LAUNCH("lov_pix_kernel");
    hipLaunchKernelGGL(lov_bwd_kernel, dim3((h * w + 255) / 256, K, B), dim3(256), 0, stream, seg, gbuf, (const float*)stats, d, outd, d_loss,
                       d_seg);
    CSEG_CHECK_LAUNCH("lov_bwd_kernel");
    return 1;
}
