// Anchor sampling on the device: the host half of hard-anchor mining (lib/loss/anchor_sampling.py:plan_selection, i.e. the keep rule of
// the reference's lib/loss/loss_contrast.py:66-82 plus its torch.randperm calls) restated as three small launches, so that the
// contrastive criterion needs no device-to-host copy and no data-dependent host value.
//
//   plan_kernel    one block. Segments s = b*K + c in image-major, class-ascending order; qual = hard + easy > max_views;
//                  T = sum qual; n_view = min(max_samples / T, max_views); every qualifying segment makes two randperm calls,
//                  (n_hard, k_hard) then (n_easy, k_easy), of max(n - 1, 0) draws each; exclusive prefixes give every segment its
//                  rank a and the offset of its first draw, and the step its `total`. Writes header, ORs the sticky status.
//   mt_kernel      one block. mt19937 with the state of torch's CPU generator (624 words + pos, csrc_host/rng_draws.cpp): advances the
//                  state by header[3] draws and writes the tempered outputs to the draw buffer.
//   pick_kernel    one thread per call: the truncated forward Fisher-Yates of csrc_host/rng_draws.cpp on a sparse image of the
//                  permutation (z = draw % (n - i)), written view-major into sel_pos / a_lab; rows >= N are -1.
//
// Everything is integer arithmetic: under the same seed the picks are those of the host path bit for bit.
#include "cseg_common.h"
#include "cseg_sampling.h"

namespace {

constexpr int MT_N = 624, MT_M = 397;

__device__ __forceinline__ uint32_t mt_twist(uint32_t u, uint32_t v) {
    return (((u & 0x80000000u) | (v & 0x7fffffffu)) >> 1) ^ ((v & 1u) ? 0x9908b0dfu : 0u);
}
__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

// One regeneration of the 624 words in LDS: four dependent phases. Inside a phase every thread reads its operands into registers, the
// block meets, and only then the new words are stored in place (word k + 1 is another thread's output).
//   k in [0, 227)    new[k] = old[k + 397] ^ twist(old[k], old[k + 1])
//   k in [227, 454)  new[k] = new[k - 227] ^ twist(old[k], old[k + 1])           (first phase)
//   k in [454, 623)  the same, new[k - 227] from the second phase
//   k = 623          new[623] = new[396] ^ twist(old[623], new[0])
__device__ __forceinline__ void mt_regenerate(uint32_t* st, int tid) {
    const int lo[4] = {0, MT_N - MT_M, 2 * (MT_N - MT_M), MT_N - 1};
    const int hi[4] = {MT_N - MT_M, 2 * (MT_N - MT_M), MT_N - 1, MT_N};
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
        const int k = lo[ph] + tid;
        const bool on = k < hi[ph];
        uint32_t v = 0;
        if (on) {
            const uint32_t far = ph == 0 ? st[k + MT_M] : st[k + MT_M - MT_N];
            const uint32_t nxt = ph == 3 ? st[0] : st[k + 1];
            v = far ^ mt_twist(st[k], nxt);
        }
        __syncthreads();
        if (on) st[k] = v;
        __syncthreads();
    }
}

// state [625] (624 words + pos), header[3] = draws of this step (0 when the step's status is set: the state stays as it is).
__global__ __launch_bounds__(SP_THREADS) void mt_kernel(uint32_t* __restrict__ state, const int32_t* __restrict__ header,
                                                        uint32_t* __restrict__ draws, int cap) {
    __shared__ uint32_t st[MT_N];
    const int tid = threadIdx.x;
    int total = header[3];
    if (total > cap) total = cap;                          // (the planner never asks for more: sum max(n - 1, 0) <= B * P)
    if (total <= 0) return;
    for (int k = tid; k < MT_N; k += SP_THREADS) st[k] = state[k];
    int pos = (int)state[MT_N];
    __syncthreads();
    for (int done = 0; done < total;) {
        if (pos >= MT_N) {
            mt_regenerate(st, tid);
            pos = 0;
        }
        const int n = min(MT_N - pos, total - done);
        for (int t = tid; t < n; t += SP_THREADS) draws[done + t] = mt_temper(st[pos + t]);
        pos += n;
        done += n;
    }
    __syncthreads();
    for (int k = tid; k < MT_N; k += SP_THREADS) state[k] = st[k];
    if (tid == 0) state[MT_N] = (uint32_t)pos;
}

// lib/loss/anchor_sampling.py:keep_rule (loss_contrast.py:66-77) in integers: x >= n_view / 2  <=>  2 x >= n_view. false = fell through.
__device__ __forceinline__ bool keep_rule(int nh, int ne, int n_view, int* kh, int* ke) {
    const bool h_ok = 2 * (long)nh >= n_view, e_ok = 2 * (long)ne >= n_view;
    if (h_ok && e_ok) {
        *kh = n_view / 2;
        *ke = n_view - *kh;
    } else if (h_ok) {
        *ke = ne;
        *kh = n_view - ne;
    } else if (e_ok) {
        *kh = nh;
        *ke = n_view - nh;
    } else {
        *kh = 0;
        *ke = 0;
        return false;
    }
    return true;
}

// seg_plan [B*K][2]: rank a of the segment among the qualifying ones (-1: does not qualify), offset of its first draw.
__global__ __launch_bounds__(SP_THREADS) void plan_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ mine_status,
                                                          int BK, int max_samples, int max_views, int draw_cap,
                                                          int32_t* __restrict__ seg_plan, int32_t* __restrict__ header,
                                                          int32_t* __restrict__ sticky) {
    __shared__ int red[SP_THREADS / 64];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const int per = (BK + SP_THREADS - 1) / SP_THREADS;
    const int s_lo = min(BK, tid * per), s_hi = min(BK, s_lo + per);
    if (tid == 0) bad = 0;
    int q = 0;
    for (int s = s_lo; s < s_hi; ++s) q += (counts[2 * s] + counts[2 * s + 1] > max_views) ? 1 : 0;
    int T;
    int a = block_excl_scan(q, red, tid, &T);
    const int n_view = T > 0 ? min(max_samples / T, max_views) : 0;
    int dr = 0;
    if (n_view > 0) {
        for (int s = s_lo; s < s_hi; ++s) {
            const int nh = counts[2 * s], ne = counts[2 * s + 1];
            if (nh + ne > max_views) {
                int kh, ke;
                if (!keep_rule(nh, ne, n_view, &kh, &ke)) bad = 1;      // (every writer stores the same value)
                dr += draws_of(nh) + draws_of(ne);
            }
        }
    }
    int total;
    int off = block_excl_scan(dr, red, tid, &total);     // (its barriers also publish `bad`)
    int status = (mine_status[0] != 0 ? 1 : 0) | (T == 0 ? 2 : 0) | ((T > 0 && n_view == 0) ? 4 : 0) | (bad ? 8 : 0);
    if (total > draw_cap) status |= 8;                    // cannot happen for counts of cseg_classify_partition (sum n <= B * P)
    for (int s = s_lo; s < s_hi; ++s) {
        const int nh = counts[2 * s], ne = counts[2 * s + 1];
        const bool qual = nh + ne > max_views;
        seg_plan[2 * s] = qual ? a : -1;
        seg_plan[2 * s + 1] = off;
        if (qual) {
            ++a;
            off += draws_of(nh) + draws_of(ne);
        }
    }
    if (tid == 0) {
        header[0] = status ? 0 : T * n_view;
        header[1] = T;
        header[2] = n_view;
        header[3] = status ? 0 : total;
        header[4] = status;
        header[5] = 0; header[6] = 0; header[7] = 0;
        sticky[0] = sticky[0] | status;
    }
}

// fy_ws [Ncap][2]: the touched positions of the permutation and what they hold, k entries per call at the call's first row
__global__ __launch_bounds__(SP_THREADS) void pick_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ seg_off,
                                                          const int32_t* __restrict__ seg_plan, const int32_t* __restrict__ header,
                                                          const uint32_t* __restrict__ draws, int BK, int K, int P, int Ncap,
                                                          int32_t* __restrict__ fy_ws, int32_t* __restrict__ sel_pos,
                                                          int32_t* __restrict__ a_lab) {
    const int gid = blockIdx.x * SP_THREADS + threadIdx.x, nthr = gridDim.x * SP_THREADS;
    const int N = header[0], T = header[1], n_view = header[2];
    for (int r = max(N, 0) + gid; r < Ncap; r += nthr) {
        sel_pos[r] = -1;
        a_lab[r] = -1;
    }
    if (N <= 0 || N > Ncap) return;
    for (int call = gid; call < 2 * BK; call += nthr) {
        const int s = call >> 1, e = call & 1;
        const int a = seg_plan[2 * s];
        if (a < 0) continue;
        const int nh = counts[2 * s], ne = counts[2 * s + 1];
        int kh, ke;
        keep_rule(nh, ne, n_view, &kh, &ke);
        const int n = e ? ne : nh, k = e ? ke : kh, v0 = e ? kh : 0;
        const uint32_t* dw = draws + seg_plan[2 * s + 1] + (e ? draws_of(nh) : 0);
        const int b = s / K, c = s - b * K;
        const int base = b * P + seg_off[2 * s + e];
        int32_t* ws = fy_ws + 2 * ((size_t)a * n_view + v0);
        const int steps = draws_of(n), kk = min(k, steps);
        int cnt = 0;
        for (int i = 0; i < kk; ++i) {
            const int zi = i + (int)(dw[i] % (uint32_t)(n - i));
            int vi = i, vj = zi, at = -1;
            for (int t = 0; t < cnt; ++t) {
                const int p = ws[2 * t], val = ws[2 * t + 1];
                if (p == i) vi = val;
                if (p == zi) { vj = val; at = t; }
            }
            const int row = (v0 + i) * T + a;
            sel_pos[row] = base + vj;                   // r[i] after the swap
            a_lab[row] = c;
            if (at < 0) {
                at = cnt++;
                ws[2 * at] = zi;
            }
            ws[2 * at + 1] = vi;
        }
        if (k > kk) {                                   // k == n: the last entry is what is left at n - 1
            int vl = n - 1;
            for (int t = 0; t < cnt; ++t)
                if (ws[2 * t] == n - 1) vl = ws[2 * t + 1];
            const int row = (v0 + kk) * T + a;
            sel_pos[row] = base + vl;
            a_lab[row] = c;
        }
    }
}

}  // namespace

extern "C" size_t cseg_sampling_ws_ints(int B, int K, int Ncap) { return (size_t)2 * B * K + (size_t)2 * Ncap; }

extern "C" int cseg_sample_anchors(const int32_t* counts, const int32_t* seg_off, const int32_t* mine_status, int B, int K, int P,
                                   int max_samples, int max_views, uint32_t* rng_state, uint32_t* draws, int32_t* ws,
                                   int32_t* sel_pos, int32_t* a_lab, int32_t* header, int32_t* sticky, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(B > 0 && K > 0 && P > 0, "sample_anchors: empty shape");
    CSEG_REQUIRE(max_samples > 0 && max_views > 0, "sample_anchors: max_samples=%d, max_views=%d", max_samples, max_views);
    CSEG_REQUIRE((size_t)B * P < ((size_t)1 << 31) && (size_t)B * K < ((size_t)1 << 29), "sample_anchors: B*P or B*K overflows int32");
    const int BK = B * K, Ncap = max_samples;
    int32_t* seg_plan = ws;
    int32_t* fy_ws = ws + 2 * (size_t)BK;
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(SP_THREADS), 0, stream, counts, mine_status, BK, max_samples, max_views, B * P,
                       seg_plan, header, sticky);
    CSEG_CHECK_LAUNCH("plan_kernel");
    hipLaunchKernelGGL(mt_kernel, dim3(1), dim3(SP_THREADS), 0, stream, rng_state, header, draws, B * P);
    CSEG_CHECK_LAUNCH("mt_kernel");
    const int work = 2 * BK > Ncap ? 2 * BK : Ncap;
    hipLaunchKernelGGL(pick_kernel, dim3((work + SP_THREADS - 1) / SP_THREADS), dim3(SP_THREADS), 0, stream, counts, seg_off, seg_plan,
                       header, draws, BK, K, P, Ncap, fy_ws, sel_pos, a_lab);
    CSEG_CHECK_LAUNCH("pick_kernel");
    return 1;
}

// The generator kernel alone (tools/device_sampling_timing.py times it; tests draw a known number of words): header[3] draws.
extern "C" int cseg_mt_draw(uint32_t* rng_state, const int32_t* header, uint32_t* draws, int cap, cseg_stream_t stream_) {
    CSEG_REQUIRE(cap > 0, "mt_draw: cap=%d", cap);
    hipLaunchKernelGGL(mt_kernel, dim3(1), dim3(SP_THREADS), 0, (hipStream_t)stream_, rng_state, header, draws, cap);
    CSEG_CHECK_LAUNCH("mt_kernel");
    return 1;
}
