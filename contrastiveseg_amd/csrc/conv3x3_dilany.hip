// 3x3 / stride 1 / padding = dilation = d convolution for ANY rate d >= 1, NCHW fp32 in and out, f16x3 split arithmetic
// (cseg_split.h), all three directions. Reference sites: the three rate-12/24/36 branches of ASPP
// (lib/models/modules/decoder_block.py: 2048 -> 512 on 65 x 129 maps) and the rate-2/4 layers of the dilated ResNets
// (lib/models/backbones/resnet/resnet_backbone.py:88-101), whose weight gradients ran on the libraries.
//
// conv3x3_sb16d_kernel (conv3x3_sb16.hip) stages a halo patch of (4 + 2d) x (64 + 2d) pixels: fine at d = 2 / 4, 28-76 patch rows
// for 4 output rows at d = 12 .. 36. Here the convolution is NINE TAP-SHIFTED 1x1 GEMMs accumulated in one launch:
//   M = a flat run of 256 pixels of the H*W plane (as in conv1x1_sb.hip), N = NT*16 output channels, K = 9 * Cin;
//   the A operand of output pixel (y, x) for tap (ky, kx) is x[b, ci, y + (ky-1) d, x + (kx-1) d], zero outside the map. Validity
//   is decided PER PIXEL from its row and column, so a flat shift that wraps over a row end reads as zero, and the width, the
//   rate, d >= H or d >= W are no special cases;
//   a tap none of whose pixels can be valid for the whole tile is skipped (block-uniform; the skipped products are exact zeros);
//   A: split while staged into the [piece][channel octet][pixel] LDS image of conv1x1_sb_kernel, double-buffered;
//   B: pre-split, pre-packed weights (CSEG_PACK_C3_ANY: tap-major slices of the 1x1 form) streamed one K-step ahead by LDS-DMA.
// Backward-data = the same kernel on the transposed packing with mirrored taps.
// Weight gradient: dW[co][ci][ky][kx] = sum_{b,y,x} dy[b,co,y,x] * x[b,ci,y+(ky-1)d,x+(kx-1)d] -- nine shifted 1x1 weight
// gradients (conv1x1_sb_wrw.hip: the contraction axis, pixels, is contiguous in both operands). A block owns one row of taps
// (ky; kx = 0, 1, 2): it stages a 32-pixel stage of dy ONCE and the three shifted x stages next to it. Stages whose output rows have
// no valid source row for this ky are not visited at all. Split-K over (image, stage) units, partials summed in a fixed order by a
// second kernel: no atomics, run-to-run bit-identical.
#include "cseg_pack.h"
#include "cseg_stats.h"

namespace {

typedef SplitF16x3 AR;
constexpr int NP = AR::NP;
constexpr int MT_PX = 256;                  // pixels per block (forward / backward-data)

__host__ __device__ constexpr int steps_any(int Cin) { return pack_steps_c1(Cin); }

// Dynamic LDS above the default limit: the attribute belongs to the (function, DEVICE) pair, so it is raised once per device
// the kernel is launched on. A failure is reported to the caller (return 0), not left to the launch.
template <auto KERNEL>
int raise_dynamic_lds(size_t lds, const char* name) {
    constexpr int MAX_DEV = 64;
    static bool done[MAX_DEV] = {};
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        cseg_set_error("%s: cannot query the current device", name);
        return 0;
    }
    const bool tracked = dev >= 0 && dev < MAX_DEV;
    if (tracked && done[dev]) return 1;
    if (hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        cseg_set_error("%s: cannot raise dynamic LDS to %zu bytes on device %d", name, lds, dev);
        return 0;
    }
    if (tracked) done[dev] = true;
    return 1;
}

__global__ __launch_bounds__(256) void pack_weights_any_kernel(const float* __restrict__ w, int Cout, int Cin, int transpose_flip,
                                                               int NT, const unsigned* __restrict__ amax_w,
                                                               uint4* __restrict__ wp, int total) {
    const float wscale = split_scale_of(split_amax_exp(amax_w));      // every thread (shuffles inside)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    pack_elem_c3_any<AR>(w, Cout, Cin, transpose_flip, NT, wscale, wp, e);
}

template <int NTW, int NTMAX>
__device__ __forceinline__ void a_kstep(const uint4* __restrict__ ap, const uint4* __restrict__ bp, f32x4 (&acc)[4][NTMAX]) {
    typedef AR::frag_t frag_t;
    frag_t a[4][NP];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int p = 0; p < NP; ++p) a[mt][p] = __builtin_bit_cast(frag_t, ap[p * 4 * MT_PX + 16 * mt]);
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        frag_t b[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) b[p] = __builtin_bit_cast(frag_t, bp[(nt * NP + p) * 64]);
#pragma unroll
        for (int t = 0; t < AR::NTERMS; ++t)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = AR::mfma(a[mt][AR::ta(t)], b[AR::tb(t)], acc[mt][nt]);
    }
}

// accumulator layout: D[m = 4*g + r][n]: pixel px0 + 16*mt + 4*g + r, channel co0 + 16*nt + n
template <int NTW, int NTMAX>
__device__ __forceinline__ void a_store_out(const f32x4 (&acc)[4][NTMAX], float* __restrict__ ybc, const float* __restrict__ bias,
                                            int co0, size_t plane, int px0, int g, int n, float unscale,
                                            const float* __restrict__ abc) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        float* orow = ybc + (size_t)(co0 + nt * 16 + n) * plane;
        const float* arow = abc ? abc + (size_t)(co0 + nt * 16 + n) * plane : nullptr;
        const float bv = bias ? bias[co0 + nt * 16 + n] : 0.f;
        const bool vec = (plane & 3) == 0;          // channel planes 16-byte aligned (else element by element: cseg_store_row4)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const long px = (long)px0 + 16 * mt + 4 * g;
            f32x4 v = acc[mt][nt] * unscale;
            v += bv;
            cseg_store_row4(orow, arow, px, (long)plane, vec, v);
        }
    }
}

// position in the sequence of K-steps: the active taps in ascending order, steps_any(Cin) K-steps each
struct StepPos {
    int mask, tap, ks;
};
__device__ __forceinline__ StepPos step_first(int mask) { return StepPos{mask, __builtin_ctz(mask), 0}; }
__device__ __forceinline__ StepPos step_next(StepPos s, int n_steps) {
    if (s.ks + 1 < n_steps) return StepPos{s.mask, s.tap, s.ks + 1};
    const int m = s.mask & (s.mask - 1);
    return StepPos{m, m ? __builtin_ctz(m) : 0, 0};
}

template <int NT>
__global__ __launch_bounds__(512, 1) void conv3x3_dilany_kernel(const float* __restrict__ x, const uint4* __restrict__ wp,
                                                                const float* __restrict__ bias, int Cin, int Cout, int H, int W,
                                                                int dil, int tiles_p, const unsigned* __restrict__ amax_x,
                                                                const unsigned* __restrict__ amax_w, float* __restrict__ y,
                                                                float4* __restrict__ stats, int n_seg, int xmap,
                                                                const float* __restrict__ addend) {
    extern __shared__ __attribute__((aligned(16))) uint4 smem_any[];
    constexpr int A1_CELLS = NP * 4 * MT_PX;       // one A buffer: [piece][octet][pixel]
    uint4* As = smem_any;                          // [2][piece NP][octet 4][MT_PX]
    uint4* Bs = smem_any + 2 * A1_CELLS;           // [2][NT*NP*64]
    constexpr int BSTEP = NT * NP * 64;
    const unsigned ex = split_amax_exp(amax_x), ew = split_amax_exp(amax_w);
    const float xscale = split_scale_of(ex);
    constexpr int NT0 = (NT + 1) / 2, NT1 = NT - NT0;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int quarter = wave & 3, half = wave >> 2;
    const int g = lane >> 4, n = lane & 15;
    const int n_cot = Cout / (NT * 16);
    const int plane_i = H * W;
    const size_t plane = (size_t)plane_i;
    // block order as in conv1x1_sb_kernel: with the XCD remap the channel tile groups that read one input tile run back to back
    int t = cseg_xcd_block(blockIdx.x, gridDim.x, xmap);
    const bool cot_first = xmap && (gridDim.x & 7) == 0;
    int cot = 0;
    if (cot_first) { cot = t % n_cot; t /= n_cot; }
    const int tp = t % tiles_p; t /= tiles_p;
    if (!cot_first) { cot = t % n_cot; t /= n_cot; }
    const int b = t;
    const int px0 = tp * MT_PX;
    const int n_steps = steps_any(Cin);
    const uint4* wbase = wp + (size_t)cot * 9 * n_steps * BSTEP;

    // taps that can have a valid source for some pixel of this tile (block-uniform). Rows: the tile's pixels lie in rows
    // y_lo .. y_hi; columns: exact when the tile lies inside one row, else "the shift fits into the row at all".
    int mask = 0;
    {
        const int q_hi = min(px0 + MT_PX, plane_i) - 1;
        const int y_lo = px0 / W, y_hi = q_hi / W;
        const int x_lo = px0 - y_lo * W, x_hi = q_hi - y_hi * W;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dyy = (tap / 3 - 1) * dil, dxx = (tap % 3 - 1) * dil;
            const bool row_ok = y_hi + dyy >= 0 && y_lo + dyy < H;
            const bool col_ok = y_lo == y_hi ? (x_hi + dxx >= 0 && x_lo + dxx < W) : dil < W || dxx == 0;
            if (row_ok && col_ok) mask |= 1 << tap;
        }
    }                                               // (the centre tap is always in)
    const int total_steps = __builtin_popcount(mask) * n_steps;

    auto b_glds = [&](StepPos s, int buf) {
        const uint4* src = wbase + ((size_t)s.tap * n_steps + s.ks) * BSTEP;
#pragma unroll
        for (int i = 0; i < (NT * NP + 7) / 8; ++i) {
            const int r = wave + 8 * i;
            if (r < NT * NP)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + r * 64 + lane),
                                                 (__attribute__((address_space(3))) void*)(Bs + buf * BSTEP + r * 64), 16, 0, 0);
        }
    };

    // A staging: item = (octet, pixel): 4 x 256 items, two per thread (octets tid >> 8 and 2 + (tid >> 8) of ONE pixel), 8 channel
    // loads each, coalesced along pixels. The pixel's row and column are fixed for the whole kernel; a tap moves them by (dyy, dxx).
    const int p_loc = tid & 255;
    const int q_pix = min(px0 + p_loc, plane_i - 1);
    const bool q_in = px0 + p_loc < plane_i;
    const int q_y = q_pix / W, q_x = q_pix - q_y * W;
    float apre[2][8];
    bool a_ok = false;
    auto a_issue = [&](StepPos s) {
        const int dyy = (s.tap / 3 - 1) * dil, dxx = (s.tap % 3 - 1) * dil;
        const int sy = q_y + dyy, sx = q_x + dxx;
        a_ok = q_in && sy >= 0 && sy < H && sx >= 0 && sx < W;
        const int sp = a_ok ? sy * W + sx : q_pix;                      // an address inside the plane either way
        const float* src = x + ((size_t)b * Cin) * plane + sp;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c0 = s.ks * 32 + ((tid >> 8) + 2 * u) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) apre[u][j] = src[(size_t)min(c0 + j, Cin - 1) * plane];      // raw; masked below
        }
    };
    auto a_put = [&](StepPos s, int buf) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int oct = (tid >> 8) + 2 * u;
            const int c0 = s.ks * 32 + oct * 8;                          // Cin % 16 == 0: an octet is inside or outside as a whole
            uint4 cells[NP];
            split_cells8_masked<AR>(apre[u], a_ok && c0 < Cin, xscale, cells);
            uint4* dst = As + buf * A1_CELLS + oct * MT_PX + p_loc;
#pragma unroll
            for (int q = 0; q < NP; ++q) dst[q * 4 * MT_PX] = cells[q];
        }
    };

    f32x4 acc[4][NT0];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT0; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    StepPos nxt = step_first(mask);                // the step being staged
    a_issue(nxt);
    b_glds(nxt, 0);
    a_put(nxt, 0);
    nxt = step_next(nxt, n_steps);
    __syncthreads();

    const uint4* a_lane = As + g * MT_PX + quarter * 64 + n;            // + buffer offset per K-step
    const uint4* b_lane = Bs + (half ? NT0 * NP * 64 : 0) + lane;
#pragma unroll 1
    for (int s = 0; s < total_steps; ++s) {
        const int buf = s & 1;
        const bool more = s + 1 < total_steps;
        if (more) {
            b_glds(nxt, buf ^ 1);                  // both stages of the other buffer were last read in step s - 1
            a_issue(nxt);
        }
        if (half == 0) a_kstep<NT0, NT0>(a_lane + buf * A1_CELLS, b_lane + buf * BSTEP, acc);
        else if (NT1 > 0) a_kstep<NT1, NT0>(a_lane + buf * A1_CELLS, b_lane + buf * BSTEP, acc);
        if (more) {
            a_put(nxt, buf ^ 1);
            nxt = step_next(nxt, n_steps);
        }
        __syncthreads();
    }

    float* ybc = y + (size_t)b * Cout * plane;
    const int co0 = cot * NT * 16;
    const float unscale = split_unscale_of(ex) * split_unscale_of(ew);
    const float* abc = addend ? addend + (size_t)b * Cout * plane : nullptr;
    if (half == 0) a_store_out<NT0, NT0>(acc, ybc, bias, co0, plane, px0 + quarter * 64, g, n, unscale, abc);
    else if (NT1 > 0) a_store_out<NT1, NT0>(acc, ybc, bias, co0 + NT0 * 16, plane, px0 + quarter * 64, g, n, unscale, abc);
    if (stats && (size_t)(px0 + quarter * 64) < plane) {      // BatchNorm statistics of what was just stored (cseg_stats.h)
        const size_t seg = (size_t)b * ((plane + 63) / 64) + (size_t)(px0 + quarter * 64) / 64;
        if (half == 0)
            cseg_stats_emit<NT0, NT0>(acc, bias, co0, unscale, px0 + quarter * 64, (long)plane, g, n, stats + (size_t)co0 * n_seg + seg, n_seg);
        else if (NT1 > 0)
            cseg_stats_emit<NT1, NT0>(acc, bias, co0 + NT0 * 16, unscale, px0 + quarter * 64, (long)plane, g, n,
                                      stats + (size_t)(co0 + NT0 * 16) * n_seg + seg, n_seg);
    }
}

// channel tiles per block: 16 for multiples of 256 from 512 on (ASPP's 512 output channels, layer4: two channel tile groups read
// every input slab instead of four), else the largest of {9, 8, 6, 4, 3} x 16 that divides Cout
int pick_nt_any(int Cout) {
    if (Cout <= 0) return 0;
    if (Cout % 256 == 0 && Cout >= 512) return 16;
    const int opts[] = {9, 8, 6, 4, 3};
    for (int nt : opts)
        if (Cout % (nt * 16) == 0) return nt;
    return 0;
}

template <int NT>
int launch_any(const float* x, const uint4* wp, const float* bias, int B, int Cin, int Cout, int H, int W, int dil,
               const unsigned* amax_x, const unsigned* amax_w, float* y, float4* stats, hipStream_t stream, const float* addend) {
    const size_t lds = sizeof(uint4) * (2 * NP * 4 * MT_PX + 2 * NT * NP * 64);
    if (!raise_dynamic_lds<conv3x3_dilany_kernel<NT>>(lds, "conv3x3_dilany")) return 0;
    const int plane = H * W;
    const int tiles_p = (plane + MT_PX - 1) / MT_PX;
    const long n_tiles = (long)B * (Cout / (NT * 16)) * tiles_p;
    CSEG_REQUIRE(n_tiles < 2147483647L, "conv3x3_dilany: grid too large");
    hipLaunchKernelGGL((conv3x3_dilany_kernel<NT>), dim3((unsigned)n_tiles), dim3(512), lds, stream, x, wp, bias, Cin, Cout, H, W, dil,
                       tiles_p, amax_x, amax_w, y, stats, B * ((plane + 63) / 64), cseg_xcd_remap(), addend);
    CSEG_CHECK_LAUNCH("conv3x3_dilany_kernel");
    return 1;
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------
constexpr int CO_T = 128, CI_T = 64, STG = 32;       // channel block, pixels per stage
constexpr int KX = 3;                                // taps per block: one row of the 3x3 (ky fixed, kx = 0, 1, 2)
constexpr int PITCH = 48;                            // half-words per (piece, channel) row: 32 + 16 pad = 96 bytes (conv1x1_sb_wrw.hip)
constexpr int DY_ELEMS = NP * CO_T * PITCH;          // one dy buffer  [piece][co 128][PITCH]
constexpr int X_ELEMS = NP * KX * CI_T * PITCH;      // one x buffer   [piece][kx 3][ci 64][PITCH]
constexpr int LD_U = (CO_T + KX * CI_T) * 8 / 512;   // 4-pixel chunks per thread and stage: 320 rows x 8 chunks / 512 threads = 5
static_assert((CO_T + KX * CI_T) * 8 == LD_U * 512 && CO_T == 2 * 64 && CI_T == 64, "item map of the weight-gradient loader");

__global__ __launch_bounds__(512, 1) void conv3x3_dilany_wrw_kernel(const float* __restrict__ x, const float* __restrict__ dy, int B,
                                                                    int Cin, int Cout, int H, int W, int dil, int n_split,
                                                                    const unsigned* __restrict__ amax_x,
                                                                    const unsigned* __restrict__ amax_dy,
                                                                    float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) unsigned short smem_anyw[];
    typedef AR::frag_t frag_t;
    unsigned short* ds = smem_anyw;                    // [2][piece][co 128][PITCH]
    unsigned short* xs = smem_anyw + 2 * DY_ELEMS;     // [2][piece][kx][ci 64][PITCH]
    const unsigned ex = split_amax_exp(amax_x), ed = split_amax_exp(amax_dy);
    const float xscale = split_scale_of(ex), dscale = split_scale_of(ed);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = lane >> 4, n = lane & 15;
    int blk = blockIdx.x;
    const int split = blk % n_split; blk /= n_split;
    const int ky = blk % 3; blk /= 3;
    const int n_cib = (Cin + CI_T - 1) / CI_T;
    const int cib = blk % n_cib;
    const int cob = blk / n_cib;
    const int plane_i = H * W;
    const size_t plane = (size_t)plane_i;
    // output rows that have a source row for this ky, and the 32-pixel stages of the plane that touch them: one contiguous range
    const int dyy = (ky - 1) * dil;
    const int y_lo = max(0, -dyy), y_hi = min(H, H - dyy);                 // [y_lo, y_hi)
    const int s_lo = y_lo < y_hi ? (y_lo * W) / STG : 0, s_hi = y_lo < y_hi ? (y_hi * W + STG - 1) / STG : 0;
    const int spi = s_hi - s_lo;                                            // active stages per image
    const long n_units = (long)B * spi;
    const long u_lo = n_units * split / n_split, u_hi = n_units * (split + 1) / n_split;

    // loader items: thread -> chunk c = tid & 7 (pixels 4c .. 4c + 3 of the stage) of rows (tid >> 3) + 64 u:
    //   u = 0, 1: dy channel cob*128 + (tid >> 3) + 64 u;   u = 2, 3, 4: x channel cib*64 + (tid >> 3), shifted for kx = u - 2
    const int c4 = 4 * (tid & 7), rloc = tid >> 3;
    const int ci_ld = cib * CI_T + rloc;
    float4 v[LD_U];
    unsigned vmask = 0;                                // bit 4u + k: pixel k of item u is inside the map
    int img = 0, stage = 0;                            // of the next stage to load (one division per block, then counted up)
    if (u_lo < u_hi) { img = (int)(u_lo / spi); stage = s_lo + (int)(u_lo % spi); }
    auto load = [&]() {
        vmask = 0;
        int q[4], qy[4], qx[4];
        const int q0 = stage * STG + c4;
        const int y0 = q0 / W, x0 = q0 - y0 * W;       // pixels behind the plane get rows >= H: masked by q < plane below
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[k] = q0 + k;
            if (W >= 4) {                              // at most one row end inside the chunk
                const bool wrap = x0 + k >= W;
                qy[k] = y0 + (wrap ? 1 : 0);
                qx[k] = x0 + k - (wrap ? W : 0);
            } else {
                qy[k] = q[k] / W;
                qx[k] = q[k] - qy[k] * W;
            }
        }
#pragma unroll
        for (int u = 0; u < LD_U; ++u) {
            float e[4];
            if (u < 2) {
                const int co = cob * CO_T + rloc + 64 * u;
                const float* row = dy + ((size_t)img * Cout + min(co, Cout - 1)) * plane;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool ok = q[k] < plane_i && co < Cout;
                    e[k] = row[min(q[k], plane_i - 1)];
                    vmask |= (ok ? 1u : 0u) << (4 * u + k);
                }
            } else {
                const int dxx = (u - 3) * dil;         // kx - 1 = u - 3
                const float* row = x + ((size_t)img * Cin + min(ci_ld, Cin - 1)) * plane;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sy = qy[k] + dyy, sx = qx[k] + dxx;
                    const bool ok = q[k] < plane_i && ci_ld < Cin && sy >= 0 && sy < H && sx >= 0 && sx < W;
                    e[k] = row[ok ? sy * W + sx : min(q[k], plane_i - 1)];
                    vmask |= (ok ? 1u : 0u) << (4 * u + k);
                }
            }
            v[u] = make_float4(e[0], e[1], e[2], e[3]);
        }
        if (++stage == s_hi) { stage = s_lo; ++img; }
    };
    auto put = [&](int buf) {
#pragma unroll
        for (int u = 0; u < LD_U; ++u) {
            float4 t = v[u];
            t.x = (vmask >> (4 * u)) & 1u ? t.x : 0.f;
            t.y = (vmask >> (4 * u + 1)) & 1u ? t.y : 0.f;
            t.z = (vmask >> (4 * u + 2)) & 1u ? t.z : 0.f;
            t.w = (vmask >> (4 * u + 3)) & 1u ? t.w : 0.f;
            uint2 cells[NP];
            split_cells4<AR>(t, u < 2 ? dscale : xscale, cells);
            unsigned short* base = u < 2 ? ds + buf * DY_ELEMS + (rloc + 64 * u) * PITCH + c4
                                         : xs + buf * X_ELEMS + ((u - 2) * CI_T + rloc) * PITCH + c4;
            const int pstride = u < 2 ? CO_T * PITCH : KX * CI_T * PITCH;
#pragma unroll
            for (int p = 0; p < NP; ++p) *reinterpret_cast<uint2*>(base + p * pstride) = cells[p];
        }
    };

    // 8 waves = 2 co halves (4 tiles of 16) x 4 ci tiles; 4 x 3 (kx) accumulators, 36 MFMAs per stage and wave
    const int mh = wave & 1, nq = wave >> 1;
    f32x4 acc[4][KX];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < KX; ++c) acc[a][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto stage_mfmas = [&](int buf) {
        frag_t bf[KX][NP];
#pragma unroll
        for (int c = 0; c < KX; ++c)
#pragma unroll
            for (int p = 0; p < NP; ++p)
                bf[c][p] = __builtin_bit_cast(frag_t, *reinterpret_cast<const uint4*>(
                    xs + buf * X_ELEMS + ((p * KX + c) * CI_T + nq * 16 + n) * PITCH + 8 * g));
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            frag_t af[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p)
                af[p] = __builtin_bit_cast(frag_t, *reinterpret_cast<const uint4*>(
                    ds + buf * DY_ELEMS + (p * CO_T + (mh * 4 + a) * 16 + n) * PITCH + 8 * g));
#pragma unroll
            for (int t = 0; t < AR::NTERMS; ++t)
#pragma unroll
                for (int c = 0; c < KX; ++c) acc[a][c] = AR::mfma(af[AR::ta(t)], bf[c][AR::tb(t)], acc[a][c]);
        }
    };

    if (u_lo < u_hi) {
        load();
        put(0);
    }
    __syncthreads();
#pragma unroll 1
    for (long unit = u_lo; unit < u_hi; ++unit) {
        const int buf = (int)(unit - u_lo) & 1;
        const bool more = unit + 1 < u_hi;
        if (more) load();
        stage_mfmas(buf);
        if (more) put(buf ^ 1);                        // that buffer was last read in the stage before (barrier since)
        __syncthreads();
    }

    // D[m = 4g + r][n]: co = cob*128 + (mh*4 + a)*16 + 4g + r, ci = cib*64 + nq*16 + n; partial[split][tap][co][ci]
    const float unscale = split_unscale_of(ex) * split_unscale_of(ed);
    const int ci = cib * CI_T + nq * 16 + n;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int co = cob * CO_T + (mh * 4 + a) * 16 + 4 * g;
#pragma unroll
        for (int c = 0; c < KX; ++c) {
            if (ci < Cin) {
                float* dst = partial + ((size_t)split * 9 + (ky * 3 + c)) * Cout * Cin;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < Cout) dst[(size_t)(co + r) * Cin + ci] = acc[a][c][r] * unscale;
            }
        }
    }
}

// dW[co][ci][tap] = sum over splits of partial[split][tap][co][ci], fixed order (the form of sb_wrw1_reduce_kernel)
__global__ __launch_bounds__(256) void dilany_wrw_reduce_kernel(const float* __restrict__ partial, int n_split, int cc, float* __restrict__ dw) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long total = 9L * cc;
    const long e = (long)blockIdx.x * 64 + lane;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (e < total) {
        int sp = wave;
        for (; sp + 12 < n_split; sp += 16) {
            s0 += partial[(size_t)sp * total + e];
            s1 += partial[(size_t)(sp + 4) * total + e];
            s2 += partial[(size_t)(sp + 8) * total + e];
            s3 += partial[(size_t)(sp + 12) * total + e];
        }
        for (; sp < n_split; sp += 4) s0 += partial[(size_t)sp * total + e];
    }
    red[wave][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (wave == 0 && e < total) {
        const long tap = e / cc, rem = e - tap * cc;
        dw[rem * 9 + tap] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    }
}

// pixel splits: one block per CU at a time (120 KB of LDS); about two rounds of blocks on 256 CUs, never more splits than stages
int wrw_any_splits(int B, int Cin, int Cout, int plane) {
    const long base = 3L * ((Cin + CI_T - 1) / CI_T) * ((Cout + CO_T - 1) / CO_T);
    const long units = (long)B * ((plane + STG - 1) / STG);
    long n = (512 + base - 1) / base;
    n = n > 64 ? 64 : n;
    n = n > units ? units : n;
    return (int)(n < 1 ? 1 : n);
}

bool shape_any_ok(int B, int Cin, int Cout, int H, int W, int dil) {
    return B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && dil >= 1 && (long)H * W < (1L << 30) && dil < (1 << 20);
}

}  // namespace

/* channel tiles per block and packing threads of a (conv_in -> conv_out) operator (0: outside the channel contract) */
extern "C" int cseg_conv3x3_split_dilany_plan(int conv_in, int conv_out, int* nt, long* threads) {
    if (!nt || !threads || conv_in <= 0 || conv_out <= 0 || conv_in % 16 || pick_nt_any(conv_out) == 0) return 0;
    *nt = pick_nt_any(conv_out);
    *threads = (long)(conv_out / 16) * 9 * steps_any(conv_in) * 64;
    return 1;
}

extern "C" size_t cseg_conv3x3_split_dilany_packed_bytes(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0 || Cin % 16 || pick_nt_any(Cout) == 0) return 0;
    return (size_t)(Cout / 16) * 9 * steps_any(Cin) * NP * 64 * sizeof(uint4);
}

extern "C" int cseg_conv3x3_split_dilany_pack(const float* w, int Cout, int Cin, int transpose_flip, const unsigned* amax_w, void* wp,
                                              cseg_stream_t stream_) {
    const int conv_in = transpose_flip ? Cout : Cin, conv_out = transpose_flip ? Cin : Cout;
    CSEG_REQUIRE(w && wp && amax_w, "conv3x3_split_dilany_pack: null pointer (f16x3 needs max|w|)");
    const int NT = pick_nt_any(conv_out);
    CSEG_REQUIRE(conv_in > 0 && conv_in % 16 == 0 && NT > 0,
                 "conv3x3_dilany: needs input channels %% 16 == 0 and output channels %% 48 == 0 or %% 64 == 0 (got %d -> %d)", conv_in,
                 conv_out);
    CSEG_REQUIRE((reinterpret_cast<uintptr_t>(wp) & 15) == 0, "conv3x3_split_dilany_pack: packed buffer must be 16-byte aligned");
    const long total = (long)(conv_out / 16) * 9 * steps_any(conv_in) * 64;
    CSEG_REQUIRE(total < 2147483647L, "conv3x3_split_dilany_pack: too large");
    hipLaunchKernelGGL(pack_weights_any_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, w, Cout, Cin,
                       transpose_flip, NT, amax_w, (uint4*)wp, (int)total);
    CSEG_CHECK_LAUNCH("conv3x3_split_dilany_pack");
    return 1;
}

extern "C" int cseg_conv3x3_split_dilany_fwd(const float* x, const void* wp, const float* bias, const float* addend, int B, int Cin,
                                             int Cout, int H, int W, int dil, const unsigned* amax_x, const unsigned* amax_w, float* y,
                                             float* stats, cseg_stream_t stream_) {
    CSEG_REQUIRE(x && wp && y && amax_x && amax_w, "conv3x3_dilany: null pointer (f16x3 needs max|x| and max|w|)");
    CSEG_REQUIRE(!(addend && stats), "conv3x3_dilany: addend and statistics cannot be combined");
    const int NT = pick_nt_any(Cout);
    CSEG_REQUIRE(shape_any_ok(B, Cin, Cout, H, W, dil) && Cin % 16 == 0 && NT > 0,
                 "conv3x3_dilany: unsupported shape B=%d Cin=%d Cout=%d H=%d W=%d dilation=%d (needs Cin %% 16 == 0, Cout %% 48 == 0 or "
                 "%% 64 == 0, dilation >= 1)", B, Cin, Cout, H, W, dil);
    CSEG_REQUIRE((reinterpret_cast<uintptr_t>(wp) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(addend) & 15) == 0 && (reinterpret_cast<uintptr_t>(stats) & 15) == 0,
                 "conv3x3_dilany: packed weights, output, addend and statistics must be 16-byte aligned");
    const uint4* wq = (const uint4*)wp;
    float4* st = reinterpret_cast<float4*>(stats);
    hipStream_t stream = (hipStream_t)stream_;
    switch (NT) {
        case 16: return launch_any<16>(x, wq, bias, B, Cin, Cout, H, W, dil, amax_x, amax_w, y, st, stream, addend);
        case 9: return launch_any<9>(x, wq, bias, B, Cin, Cout, H, W, dil, amax_x, amax_w, y, st, stream, addend);
        case 8: return launch_any<8>(x, wq, bias, B, Cin, Cout, H, W, dil, amax_x, amax_w, y, st, stream, addend);
        case 6: return launch_any<6>(x, wq, bias, B, Cin, Cout, H, W, dil, amax_x, amax_w, y, st, stream, addend);
        case 4: return launch_any<4>(x, wq, bias, B, Cin, Cout, H, W, dil, amax_x, amax_w, y, st, stream, addend);
        default: return launch_any<3>(x, wq, bias, B, Cin, Cout, H, W, dil, amax_x, amax_w, y, st, stream, addend);
    }
}

extern "C" size_t cseg_conv3x3_split_dilany_wrw_ws_floats(int B, int Cin, int Cout, int H, int W, int dil) {
    if (!shape_any_ok(B, Cin, Cout, H, W, dil) || Cin % 16 || Cout % 16) return 0;
    return (size_t)wrw_any_splits(B, Cin, Cout, H * W) * 9 * Cin * Cout;
}

extern "C" int cseg_conv3x3_split_dilany_wrw(const float* x, const float* dy, int B, int Cin, int Cout, int H, int W, int dil,
                                             const unsigned* amax_x, const unsigned* amax_dy, float* ws, float* dw,
                                             cseg_stream_t stream_) {
    CSEG_REQUIRE(x && dy && ws && dw && amax_x && amax_dy, "conv3x3_dilany_wrw: null pointer (f16x3 needs max|x| and max|dy|)");
    CSEG_REQUIRE(shape_any_ok(B, Cin, Cout, H, W, dil) && Cin % 16 == 0 && Cout % 16 == 0,
                 "conv3x3_dilany_wrw: unsupported shape B=%d Cin=%d Cout=%d H=%d W=%d dilation=%d (needs channels %% 16, dilation >= 1)",
                 B, Cin, Cout, H, W, dil);
    hipStream_t stream = (hipStream_t)stream_;
    const int n_split = wrw_any_splits(B, Cin, Cout, H * W);
    const long blocks = (long)n_split * 3 * ((Cin + CI_T - 1) / CI_T) * ((Cout + CO_T - 1) / CO_T);
    CSEG_REQUIRE(blocks < 2147483647L && 9L * Cin * Cout < 2147483647L, "conv3x3_dilany_wrw: grid too large");
    const size_t lds = sizeof(unsigned short) * 2 * (DY_ELEMS + X_ELEMS);
    if (!raise_dynamic_lds<conv3x3_dilany_wrw_kernel>(lds, "conv3x3_dilany_wrw")) return 0;
    hipLaunchKernelGGL(conv3x3_dilany_wrw_kernel, dim3((unsigned)blocks), dim3(512), lds, stream, x, dy, B, Cin, Cout, H, W, dil, n_split,
                       amax_x, amax_dy, ws);
    CSEG_CHECK_LAUNCH("conv3x3_dilany_wrw_kernel");
    const long total = 9L * Cin * Cout;
    hipLaunchKernelGGL(dilany_wrw_reduce_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, stream, ws, n_split, Cin * Cout, dw);
    CSEG_CHECK_LAUNCH("dilany_wrw_reduce_kernel");
    return 1;
}
