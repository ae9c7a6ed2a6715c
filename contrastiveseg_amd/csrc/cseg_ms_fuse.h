// The test phase's multi-scale + flip fusion kernel, one text for its two launch shapes: MsArgs, a [B,K,H,W] batch (ms_eval.hip,
// cseg_ms_fuse_argmax), and RgArgs, images of differing sizes with packed outputs (ms_eval_ragged.hip, cseg_ms_fuse_argmax_ragged). The
// two differ in which image and pixel a thread owns and where its byte and its fp32 column go, which is decided at compile time; the
// taps and the class loop are the same statements, so a pixel (y, x) of a W-wide map gets the same operations from both. Two further
// argument types ride on them: MsPermuted<Base> (a channel permutation on the mirrored operand, cseg_ms_fuse_argmax_perm / _ragged_perm)
// and MsWeighted<MsArgs> (a per-pixel weight per term, cseg_ms_fuse_argmax_weighted in ms_eval.hip).
#pragma once
#include <type_traits>

#include "cseg_taps.h"

namespace {

constexpr int MS_MAX_TERMS = 8;
constexpr int MS_MAX_K = 256;
constexpr int RG_IMAGES = 8;             // images per ragged launch: RgArgs stays under HIP's 4 KB of kernel arguments

struct MsTerm {
    const float* a;      // [B,K,h,w]
    const float* b;      // [B,K,h,w] net output for the mirrored input, or null
    int h, w;
    float sy, sx, wt;
};

struct MsArgs {
    MsTerm t[MS_MAX_TERMS];
    int n, B, K, H, W;
};

struct RgImage {
    long pix0;           // pixels of the images before this one in the packed outputs
    int W;               // padded width: the geometry's, and the mirror's
    int w;               // border width: the row length of this image's outputs
    int npix;            // h * w of the border
    int block0;          // first block of this image in the launch
};

struct RgArgs {          // maps of one image: [1,K,h,w]
    MsTerm t[RG_IMAGES][MS_MAX_TERMS];
    RgImage im[RG_IMAGES];
    int n_images, n, K;
};
static_assert(sizeof(RgArgs) + 2 * sizeof(void*) <= 4096, "the argument block of the ragged launch exceeds HIP's 4 KB");

// The channel permutation of the mirrored operand (left/right classes under a flip; cseg_ms_fuse_argmax_perm, _ragged_perm): output
// class k reads class perm[k] of every flipped map. The table travels in the argument block behind the descriptors, one byte per
// class packed into dwords, so that the class loop's look-up is a scalar dword load and a shift, both wave-uniform. An argument
// block WITH a table is its own type: the instances of MsArgs and RgArgs themselves compile from the text they always had.
struct MsPerm {
    uint32_t w[MS_MAX_K / 4];
    void fill(const uint8_t* perm, int K) {              // host: the K entries, zeros behind them
        for (int j = 0; j < MS_MAX_K / 4; ++j) w[j] = 0u;
        for (int k = 0; k < K; ++k) w[k >> 2] |= (uint32_t)perm[k] << ((k & 3) * 8);
    }
    __device__ __forceinline__ int get(int k) const { return (int)((w[k >> 2] >> ((k & 3) * 8)) & 255u); }
};
template <class Base>
struct MsPermuted : Base {
    MsPerm perm;
};
template <class Args> struct ms_is_permuted : std::false_type {};
template <class Base> struct ms_is_permuted<MsPermuted<Base>> : std::true_type {};
static_assert(sizeof(MsPermuted<RgArgs>) + 2 * sizeof(void*) <= 4096, "the permuted ragged argument block exceeds HIP's 4 KB");

// Per-pixel term weights (depth-aware fusion, segmentor/tester.py:447-475 of the reference; cseg_ms_fuse_argmax_weighted): pixel g of
// the batch carries a bin, bins[g], and term i weighs its sum there with table[i * nbins + bin] in place of t[i].wt. Both arrays stay
// in global memory -- n loads per pixel ahead of the class loop, from a table of at most 8 x 16 floats that lives in L1 -- so there is
// no LDS copy and no barrier, and the early return of the threads behind the last pixel stays legal. An argument block WITH pixel
// weights is its own type, as with MsPermuted. MS_MAX_BINS bounds nbins; a bin >= nbins reads column nbins - 1.
constexpr int MS_MAX_BINS = 16;
struct MsPixelWeights {
    const uint8_t* bins;     // [B,H,W]
    const float* table;      // [n, nbins]
    int nbins;
};
template <class Base>
struct MsWeighted : Base {
    MsPixelWeights pw;
};
template <class Args> struct ms_is_weighted : std::false_type {};
template <class Base> struct ms_is_weighted<MsWeighted<Base>> : std::true_type {};

// perm[0..K) must be a permutation of 0..K-1. -> null, or what is wrong with it (entry index and value in *at, *val).
inline const char* ms_perm_fault(const uint8_t* perm, int K, int* at, int* val) {
    bool seen[MS_MAX_K] = {};
    for (int k = 0; k < K; ++k) {
        *at = k; *val = perm[k];
        if (perm[k] >= K) return "is not a class";
        if (seen[perm[k]]) return "repeats an earlier entry (not a permutation)";
        seen[perm[k]] = true;
    }
    return nullptr;
}

// The weight of bl_tap's upper tap with its one rounding stated: fma(s, o, -i0) when FUSED, else the rounded product minus i0.
// bl_tap itself is compiled under the default contraction, which leaves that choice to the optimiser, instance by instance.
template <bool FUSED>
__device__ __forceinline__ float ms_tap_weight(float s, int o, int i0) {
#pragma clang fp contract(off)
    return FUSED ? fmaf(s, (float)o, -(float)i0) : s * (float)o - (float)i0;
}

// Which of the two the MsArgs instances -- what cseg_ms_fuse_argmax has always run -- got from the optimiser. On the GPU: the weight
// of the mirrored column fused in every instance; the row weight and the plain column's weight fused in the one-term instance only
// (from two terms on the products s * y and s * x are one packed multiply, which keeps them from fusing). In a host build of this
// text (the CPU emulation of the tests) nothing is fused.
#if defined(__HIP_DEVICE_COMPILE__)
template <int NT> constexpr bool MS_PLAIN_WEIGHTS_FUSED = NT == 1;
constexpr bool MS_MIRROR_WEIGHT_FUSED = true;
#else
template <int NT> constexpr bool MS_PLAIN_WEIGHTS_FUSED = false;
constexpr bool MS_MIRROR_WEIGHT_FUSED = false;
#endif

// MsArgs: one thread per output pixel of the batch. RgArgs: one thread per pixel of an image's border; image j owns the blocks from
// im[j].block0 on, so the block-to-image map and every descriptor read are wave-uniform. MsPermuted<MsArgs>, MsPermuted<RgArgs>: the
// same two with the flipped maps' classes permuted (a compile-time property of the argument type). MsWeighted<MsArgs>: the batch
// form with the term weights read per pixel.
template <int NT, class Args>
__global__ __launch_bounds__(256) void ms_fuse_kernel(Args A, uint8_t* __restrict__ pred, float* __restrict__ fused) {
#pragma clang fp contract(off)
    constexpr bool ragged = std::is_base_of<RgArgs, Args>::value;
    constexpr bool permuted = ms_is_permuted<Args>::value;
    constexpr bool weighted = ms_is_weighted<Args>::value;
    long g, HW;
    int b, p, y, x, xm;
    const MsTerm* t;
    if constexpr (ragged) {
        int img = 0;
#pragma unroll
        for (int j = 1; j < RG_IMAGES; ++j)
            if (j < A.n_images && (int)blockIdx.x >= A.im[j].block0) img = j;
        p = ((int)blockIdx.x - A.im[img].block0) * 256 + (int)threadIdx.x;
        if (p >= A.im[img].npix) return;
        HW = A.im[img].npix;
        g = A.im[img].pix0 + p;
        b = 0;
        y = p / A.im[img].w; x = p - y * A.im[img].w;
        xm = A.im[img].W - 1 - x;
        t = A.t[img];
        if (fused) fused += (size_t)A.K * (size_t)A.im[img].pix0;          // this image's [K,h,w] block
    } else {
        g = (long)blockIdx.x * 256 + threadIdx.x;
        HW = (long)A.H * A.W;
        if (g >= (long)A.B * HW) return;
        b = (int)(g / HW);
        p = (int)(g - (long)b * HW);
        y = p / A.W; x = p - y * A.W;
        xm = A.W - 1 - x;
        t = A.t;
    }

    int r0[NT], r1[NT], xa0[NT], xa1[NT], xb0[NT], xb1[NT];
    float ly[NT], lxa[NT], lxb[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        r0[i] = r1[i] = xa0[i] = xa1[i] = xb0[i] = xb1[i] = 0;
        ly[i] = lxa[i] = lxb[i] = 0.f;
        if (i < A.n) {
            int y0, y1;
            bl_tap(t[i].sy, t[i].h, y, y0, y1, ly[i]);
            bl_tap(t[i].sx, t[i].w, x, xa0[i], xa1[i], lxa[i]);
            bl_tap(t[i].sx, t[i].w, xm, xb0[i], xb1[i], lxb[i]);
            if constexpr (ragged || permuted || weighted) {
                // The ragged and the permuted instances must give the bits of the MsArgs instances image by image, so they state the
                // roundings of the tap weights instead of leaving them to a second, independent choice of the optimiser; the tests
                // compare the two bit for bit, on the GPU and on the emulation (tests/test_gpu_ms_eval_ragged.py,
                // tests/test_emu_ms_eval_ragged.py; the permuted ones against the plain call on gathered maps,
                // tests/test_gpu_lip_swap.py; the weighted ones with a table that is constant per term against the plain call with
                // those constants as scalar weights, tests/test_gpu_ms_depth.py).
                ly[i] = ms_tap_weight<MS_PLAIN_WEIGHTS_FUSED<NT>>(t[i].sy, y, y0);
                lxa[i] = ms_tap_weight<MS_PLAIN_WEIGHTS_FUSED<NT>>(t[i].sx, x, xa0[i]);
                lxb[i] = ms_tap_weight<MS_MIRROR_WEIGHT_FUSED>(t[i].sx, xm, xb0[i]);
            }
            // the fp32 source coordinate of the last output index is at most n_in - 1 + rounding, so these change no tap; they
            // make every address provably inside the plane
            y0 = min(y0, t[i].h - 1); y1 = min(y1, t[i].h - 1);
            xa0[i] = min(xa0[i], t[i].w - 1); xa1[i] = min(xa1[i], t[i].w - 1);
            xb0[i] = min(xb0[i], t[i].w - 1); xb1[i] = min(xb1[i], t[i].w - 1);
            r0[i] = y0 * t[i].w;
            r1[i] = y1 * t[i].w;
        }
    }

    float wpx[weighted ? NT : 1];        // the weighted instances: this pixel's weight of every term
    if constexpr (weighted) {
        const int bin = min((int)A.pw.bins[g], A.pw.nbins - 1);
#pragma unroll
        for (int i = 0; i < NT; ++i) wpx[i] = i < A.n ? A.pw.table[i * A.pw.nbins + bin] : 0.f;
    }

    float best = 0.f;
    int best_k = 0;
    for (int k = 0; k < A.K; ++k) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if (i < A.n) {
                const size_t plane = ((size_t)b * A.K + k) * ((size_t)t[i].h * t[i].w);
                const float ly1 = ly[i], ly0 = 1.f - ly1;
                const float* s = t[i].a + plane;
                float c0 = ly0 * s[r0[i] + xa0[i]] + ly1 * s[r1[i] + xa0[i]];
                float c1 = ly0 * s[r0[i] + xa1[i]] + ly1 * s[r1[i] + xa1[i]];
                float u = fmaf(lxa[i], c1 - c0, c0);
                if (t[i].b) {
                    if constexpr (permuted)     // output class k reads class perm[k] of the mirrored operand
                        s = t[i].b + ((size_t)b * A.K + A.perm.get(k)) * ((size_t)t[i].h * t[i].w);
                    else
                        s = t[i].b + plane;
                    c0 = ly0 * s[r0[i] + xb0[i]] + ly1 * s[r1[i] + xb0[i]];
                    c1 = ly0 * s[r0[i] + xb1[i]] + ly1 * s[r1[i] + xb1[i]];
                    u = u + fmaf(lxb[i], c1 - c0, c0);
                }
                if constexpr (weighted)
                    v = v + wpx[i] * u;
                else
                    v = v + t[i].wt * u;
            }
        }
        if (fused) fused[((size_t)b * A.K + k) * HW + p] = v;
        if (k == 0 || v > best) { best = v; best_k = k; }
    }
    if (pred) pred[g] = (uint8_t)best_k;
}

}  // namespace
