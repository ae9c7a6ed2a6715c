// The classifier convolution for 33 .. 256 classes (COCO-Stuff 171, ADE20K 150, Pascal-Context 60): the same three operators and the
// same per-image weight layout as csrc/cls1x1.hip (wt [B][C][KP], Dropout2d mask folded in, pad columns zero), but no longer streams:
// 2 K flops per 4 bytes of the wide activation is compute-bound on fp32 from a few dozen classes on, so these are fp32 GEMMs on the
// fp32-input matrix instruction v_mfma_f32_32x32x2_f32. Its result is bit for bit a k-ordered fmaf chain (one rounding per product, no
// wider accumulation): the logits stay exact fp32, in another summation order than the library's.
//   forward        y[b][k][p]  = bias[k] + sum_c wt[b][c][k] x[b][c][p]
//   backward-data  dx[b][c][p] = sum_k wt[b][c][k] dy[b][k][p]
//   weight grad.   dwt[b][c][k] = sum_p x[b][c][p] dy[b][k][p]
// KP = K rounded up to a multiple of 32 (kernels.cls1x1_wide_kp), NT = KP / 32 class tiles (2 .. 8) is the template parameter.
// Operand maps of the instruction (lane l, r = l & 31, h = l >> 5): A[i = r][k = h], B[k = h][j = r], one VGPR each;
// D[i][j]: lane j + 32 ((i / 4) % 2), register i % 4 + 4 (i / 8) -- the column on the lane, so a store of one register is 32 consecutive
// floats of one row.
// Every operator reads the wide tensor once:
//   forward        block = 128 pixels x all KP classes, wave = 32 pixels. x is the B operand straight from global memory (32 consecutive
//                  pixels of two channels per wave load); the weights go through LDS in chunks of 32 channels.
//   backward-data  wave = 32 pixels with their dy in registers (KP / 2 per lane) as the B operand; 32-channel tiles of wt through LDS.
//   weight grad.   block = 128 channels x all KP classes x a split of the pixels, wave = 32 channels. x and dy are contiguous along the
//                  reduction axis, so both are transposed through LDS ([row][pixel], pitch 34: the lane = row reads are conflict-free);
//                  partial sums per split, added in split order by a second kernel.
// All sums in a fixed order (no atomics): deterministic. Any P and any C: ragged tiles load zeros and skip the stores.
#include "cseg_common.h"
#include "cseg_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CC = 32;                 // channels per LDS chunk / tile
constexpr int PXB = 128;               // pixels per block (forward, backward-data): 4 waves x 32

// row of D held in register v by lane half h
__device__ __forceinline__ int d_row(int v, int h) { return (v & 3) + 8 * (v >> 2) + 4 * h; }

// ---- forward -------------------------------------------------------------------------------------------------------------------------
// Ws[c][k], pitch = 32 (mod 64) floats: the two lane halves (channels c, c + 1) read from the two halves of the banks
template <int NT>
__global__ __launch_bounds__(256) void cls1x1_wide_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                              const float* __restrict__ bias, int C, int K, long P, int tiles,
                                                              float* __restrict__ y) {
    constexpr int KP = NT * 32, PITCH = (NT | 1) * 32, WREG = NT * 4;       // 32 x KP floats over 256 threads
    __shared__ float Ws[CC * PITCH];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long p = (long)tile * PXB + wave * 32 + r;
    const bool live = p < P;
    const float* xp = x + (size_t)b * C * P + (live ? p : P - 1);
    const float* wp = wt + (size_t)b * C * KP;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;
    float wreg[WREG], xreg[CC / 2];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int q = 0; q < WREG; ++q) {
            const int idx = tid + 256 * q, c = c0 + idx / KP;              // the chunk is contiguous in wt: coalesced
            wreg[q] = c < C ? wp[(size_t)c0 * KP + idx] : 0.f;
        }
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
        float a[NT], an[NT];                                   // the A operands of step s + 1 are read under the NT instructions of step s
#pragma unroll
        for (int t = 0; t < NT; ++t) a[t] = Ws[h * PITCH + t * 32 + r];
#pragma unroll
        for (int s = 0; s < CC / 2; ++s) {
            if (s + 1 < CC / 2) {
#pragma unroll
                for (int t = 0; t < NT; ++t) an[t] = Ws[(2 * s + 2 + h) * PITCH + t * 32 + r];
            }
            __builtin_amdgcn_sched_barrier(0);                 // (the scheduler otherwise sinks each read to just in front of its use)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], xcur[s], acc[t], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NT; ++t) a[t] = an[t];
        }
    }
    if (live) {
        float* yp = y + (size_t)b * K * P + p;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int k = t * 32 + d_row(v, h);
                if (k < K) yp[(size_t)k * P] = acc[t][v] + (bias ? bias[k] : 0.f);
            }
    }
}

// ---- backward-data -------------------------------------------------------------------------------------------------------------------
// Wt[c][k], pitch = KP + 2 = 2 or 34 (mod 64): lane (c = r, class 2 kk + h) reads bank 2 r + h (+ 32 for odd r): conflict-free
template <int NT>
__global__ __launch_bounds__(256) void cls1x1_wide_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ wt, int C, int K,
                                                              long P, int tiles, float* __restrict__ dx) {
    constexpr int KP = NT * 32, PITCH = KP + 2, WREG = NT * 4;
    __shared__ float Wt[CC * PITCH];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const long p = (long)tile * PXB + wave * 32 + r;
    const bool live = p < P;
    const long pc = live ? p : P - 1;
    float d[KP / 2];                                           // B operand of step kk: dy[class 2 kk + h][pixel r]
#pragma unroll
    for (int kk = 0; kk < KP / 2; ++kk) {
        const int k = 2 * kk + h;
        d[kk] = k < K ? dy[((size_t)b * K + k) * P + pc] : 0.f;
    }
    const int c_tiles = (C + CC - 1) / CC;
    const int per = (c_tiles + (int)gridDim.y - 1) / (int)gridDim.y;
    const int t0 = blockIdx.y * per, t1 = min(c_tiles, t0 + per);
    const float* wp = wt + (size_t)b * C * KP;
    float wreg[WREG];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int q = 0; q < WREG; ++q) {
            const int idx = tid + 256 * q, c = c0 + idx / KP;
            wreg[q] = c < C ? wp[(size_t)c0 * KP + idx] : 0.f;
        }
    };
    if (t0 < t1) fetch(t0 * CC);
    for (int ct = t0; ct < t1; ++ct) {
        const int c0 = ct * CC;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < WREG; ++q) {
            const int idx = tid + 256 * q;
            Wt[(idx / KP) * PITCH + idx % KP] = wreg[q];
        }
        __syncthreads();
        if (ct + 1 < t1) fetch(c0 + CC);
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
            __builtin_amdgcn_sched_barrier(0);                 // (the scheduler otherwise sinks each read to just in front of its use)
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

// ---- weight gradient -----------------------------------------------------------------------------------------------------------------
constexpr int WCB = 128;               // channels per block: 4 waves x 32
constexpr int WPS = 32;                // pixels per stage
constexpr int T_PITCH = WPS + 2;       // [row][pixel]: lane (row r, pixel 2 s + h) reads bank 34 r + h (mod 64): conflict-free

template <int NT, bool VEC>
__global__ __launch_bounds__(256) void cls1x1_wide_wrw_kernel(const float* __restrict__ x, const float* __restrict__ dy, int C, int K,
                                                              long P, int c_tiles, int n_split, int B, float* __restrict__ partial) {
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

// dwt[e] = sum over the splits, in order
__global__ __launch_bounds__(256) void cls1x1_wide_wrw_reduce_kernel(const float* __restrict__ partial, int n_split, long total,
                                                                     float* __restrict__ dwt) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = 0.f;
    for (int sp = 0; sp < n_split; ++sp) s += partial[(size_t)sp * total + e];
    dwt[e] = s;
}

int wide_wrw_splits(int B, int C, int KP, long P) {
    const long stages = (P + WPS - 1) / WPS;
    const long groups = (long)B * ((C + WCB - 1) / WCB);
    // one round of resident blocks, not one and a half: a block is one wave per SIMD, and the registers of the NT = KP / 32 accumulator
    // tiles allow 4 / 2 / 1 of them per SIMD on 256 CUs
    const long resident = 256 * (KP <= 96 ? 4 : KP <= 224 ? 2 : 1);
    long n = resident / groups;
    if (n > stages) n = stages;
    if (n > 64) n = 64;
    return (int)(n < 1 ? 1 : n);
}

bool wide_shape_ok(int B, int C, int K, int KP, long P) {
    return B > 0 && C > 0 && K > 32 && K <= 256 && KP == (K + 31) / 32 * 32 && P > 0 && (long)B * C * P < (1L << 40) &&
           (long)B * ((P + PXB - 1) / PXB) < 2147483647L / 16;
}

#define WIDE_DISPATCH(NTV, CALL)                                                                                                      \
    switch (NTV) {                                                                                                                    \
        case 2: CALL(2); break;                                                                                                       \
        case 3: CALL(3); break;                                                                                                       \
        case 4: CALL(4); break;                                                                                                       \
        case 5: CALL(5); break;                                                                                                       \
        case 6: CALL(6); break;                                                                                                       \
        case 7: CALL(7); break;                                                                                                       \
        default: CALL(8); break;                                                                                                      \
    }

}  // namespace

extern "C" int cseg_cls1x1_wide_fwd(const float* x, const float* wt, const float* bias, int B, int C, int K, int KP, long P, float* y,
                                    cseg_stream_t stream_) {
    CSEG_REQUIRE(x && wt && y, "cls1x1_wide_fwd: null pointer");
    CSEG_REQUIRE(wide_shape_ok(B, C, K, KP, P),
                 "cls1x1_wide_fwd: unsupported shape B=%d C=%d K=%d KP=%d P=%ld (32 < K <= 256, KP = K rounded up to 32)", B, C, K, KP, P);
    hipStream_t stream = (hipStream_t)stream_;
    const int tiles = (int)((P + PXB - 1) / PXB);
#define CLS_FWD(NTV)                                                                                                                  \
    hipLaunchKernelGGL(cls1x1_wide_fwd_kernel<NTV>, dim3((unsigned)(B * tiles)), dim3(256), 0, stream, x, wt, bias, C, K, P, tiles, y)
    WIDE_DISPATCH(KP / 32, CLS_FWD)
#undef CLS_FWD
    CSEG_CHECK_LAUNCH("cls1x1_wide_fwd_kernel");
    return 1;
}

extern "C" int cseg_cls1x1_wide_bwd(const float* dy, const float* wt, int B, int C, int K, int KP, long P, float* dx,
                                    cseg_stream_t stream_) {
    CSEG_REQUIRE(dy && wt && dx, "cls1x1_wide_bwd: null pointer");
    CSEG_REQUIRE(wide_shape_ok(B, C, K, KP, P),
                 "cls1x1_wide_bwd: unsupported shape B=%d C=%d K=%d KP=%d P=%ld (32 < K <= 256, KP = K rounded up to 32)", B, C, K, KP, P);
    hipStream_t stream = (hipStream_t)stream_;
    const int tiles = (int)((P + PXB - 1) / PXB), c_tiles = (C + CC - 1) / CC;
    int parts = 1;                                             // channel parts: enough blocks for the chip (each re-reads its pixels' dy)
    while (parts < 16 && (long)B * tiles * parts < 1024 && c_tiles / (parts * 2) >= 2) parts *= 2;
#define CLS_BWD(NTV)                                                                                                                  \
    hipLaunchKernelGGL(cls1x1_wide_bwd_kernel<NTV>, dim3((unsigned)(B * tiles), parts), dim3(256), 0, stream, dy, wt, C, K, P, tiles, dx)
    WIDE_DISPATCH(KP / 32, CLS_BWD)
#undef CLS_BWD
    CSEG_CHECK_LAUNCH("cls1x1_wide_bwd_kernel");
    return 1;
}

extern "C" size_t cseg_cls1x1_wide_wrw_ws_floats(int B, int C, int KP, long P) {
    if (B <= 0 || C <= 0 || P <= 0 || KP < 64 || KP > 256 || KP % 32 != 0) return 0;
    return (size_t)wide_wrw_splits(B, C, KP, P) * B * C * KP;
}

extern "C" int cseg_cls1x1_wide_wrw(const float* x, const float* dy, int B, int C, int K, int KP, long P, float* ws, float* dwt,
                                    cseg_stream_t stream_) {
    CSEG_REQUIRE(x && dy && ws && dwt, "cls1x1_wide_wrw: null pointer");
    CSEG_REQUIRE(wide_shape_ok(B, C, K, KP, P),
                 "cls1x1_wide_wrw: unsupported shape B=%d C=%d K=%d KP=%d P=%ld (32 < K <= 256, KP = K rounded up to 32)", B, C, K, KP, P);
    hipStream_t stream = (hipStream_t)stream_;
    const int n_split = wide_wrw_splits(B, C, KP, P), c_tiles = (C + WCB - 1) / WCB;
    const long blocks = (long)B * c_tiles * n_split;
    CSEG_REQUIRE(blocks < 2147483647L, "cls1x1_wide_wrw: grid too large");
    const bool vec = P % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy)) & 15) == 0;
#define CLS_WRW(NTV)                                                                                                                  \
    do {                                                                                                                              \
        if (vec)                                                                                                                      \
            hipLaunchKernelGGL((cls1x1_wide_wrw_kernel<NTV, true>), dim3((unsigned)blocks), dim3(256), 0, stream, x, dy, C, K, P,     \
                               c_tiles, n_split, B, ws);                                                                              \
        else                                                                                                                          \
            hipLaunchKernelGGL((cls1x1_wide_wrw_kernel<NTV, false>), dim3((unsigned)blocks), dim3(256), 0, stream, x, dy, C, K, P,    \
                               c_tiles, n_split, B, ws);                                                                              \
    } while (0)
    WIDE_DISPATCH(KP / 32, CLS_WRW)
#undef CLS_WRW
    CSEG_CHECK_LAUNCH("cls1x1_wide_wrw_kernel");
    const long total = (long)B * C * KP;
    hipLaunchKernelGGL(cls1x1_wide_wrw_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ws, n_split, total, dwt);
    CSEG_CHECK_LAUNCH("cls1x1_wide_wrw_reduce_kernel");
    return 1;
}
