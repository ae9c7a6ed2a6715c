// Test phase on mixed-size datasets: the multi-scale + flip fusion with the argmax for a RAGGED batch, one launch.
// Reference: segmentor/tester.py:328-341 (ss_test, list branch: every image alone, padded right / down to fit_stride, the net's output
// interpolated back to the PADDED size), :400-421 (ms_test, list branch: full += weight * (probs + flip(flip_probs, 3)); the mirrored
// input is the flip of the padded tensor, so its padding lies on the left) and :169-189 (the crop [:border_h, :border_w], top-left,
// then the argmax). lib/datasets/tools/collate.py:61-68, 107-146 for the padding.
//
// ms_fuse_kernel<NT, RgArgs> of cseg_ms_fuse.h: one thread per pixel of an image's BORDER (its unpadded h_b x w_b region), so pad pixels
// are never computed. Blocks are dealt out image by image -- image b owns ceil(h_b * w_b / 256) consecutive blocks -- so the
// block-to-image map and every descriptor read are wave-uniform (scalar loads from the argument block). The geometry is that of the
// PADDED map: scales ac_scale(hc, Hp_b) / ac_scale(wc, Wp_b), mirrored column Wp_b - 1 - x. Taps and class loop are the statements
// cseg_ms_fuse_argmax's instance of the same template runs: image b's pixels carry the bits it gives for that image at (Hp_b, Wp_b).
// Outputs are packed: pred holds the images one after the other, each h_b * w_b bytes row-major; fused is image-major, then
// [K, h_b, w_b]. No atomics, no LDS: deterministic.
// Descriptors travel by value, RG_IMAGES images x MS_MAX_TERMS terms per launch (under HIP's 4 KB of kernel arguments): a batch of
// up to RG_IMAGES images is one launch, a larger one ceil(n / RG_IMAGES) launches on the same stream.
#include "cseg_ms_fuse.h"

// cseg_ms_fuse_argmax_ragged_perm: the flipped maps' classes permuted as in cseg_ms_fuse_argmax_perm (one table for the batch), the
// MsPermuted<RgArgs> instances; a null table launches the instances the entry point without it always has.
extern "C" int cseg_ms_fuse_argmax_ragged_perm(int n_images, int n_terms, const float* const* plain, const float* const* flipped,
                                               const int* hs, const int* ws, const float* weights, const uint8_t* perm,
                                               const int* geometry, int K, uint8_t* pred, float* fused, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(n_images >= 1 && n_images <= 65535, "ms_fuse_argmax_ragged: %d images (1 to 65535 are supported)", n_images);
    CSEG_REQUIRE(n_terms >= 1 && n_terms <= MS_MAX_TERMS, "ms_fuse_argmax_ragged: %d terms (1 to %d are supported)", n_terms,
                 MS_MAX_TERMS);
    CSEG_REQUIRE(plain && hs && ws && weights && geometry, "ms_fuse_argmax_ragged: null term or geometry arrays");
    CSEG_REQUIRE(K >= 1 && K <= MS_MAX_K, "ms_fuse_argmax_ragged: %d classes (the prediction is one byte; 1 to %d)", K, MS_MAX_K);
    CSEG_REQUIRE(pred || fused, "ms_fuse_argmax_ragged: both outputs are null");
    // everything is checked before the first launch: a refused batch writes nothing
    long total = 0;
    for (int b = 0; b < n_images; ++b) {
        const int Hp = geometry[4 * b], Wp = geometry[4 * b + 1], h = geometry[4 * b + 2], w = geometry[4 * b + 3];
        CSEG_REQUIRE(Hp > 0 && Wp > 0 && h > 0 && w > 0, "ms_fuse_argmax_ragged: image %d is empty (padded %d x %d, border %d x %d)", b,
                     Hp, Wp, h, w);
        CSEG_REQUIRE(h <= Hp && w <= Wp, "ms_fuse_argmax_ragged: image %d: the border %d x %d exceeds the padded size %d x %d", b, h, w,
                     Hp, Wp);
        total += (long)h * w;
        CSEG_REQUIRE(total < 2147483648L && total * K < 2147483648L,
                     "ms_fuse_argmax_ragged: the packed outputs up to image %d (%ld pixels, %d classes) do not fit 31 bits", b, total, K);
        for (int i = 0; i < n_terms; ++i) {
            const int e = b * n_terms + i;
            CSEG_REQUIRE(plain[e], "ms_fuse_argmax_ragged: term %d of image %d has no plain map", i, b);
            CSEG_REQUIRE(hs[e] > 0 && ws[e] > 0, "ms_fuse_argmax_ragged: term %d of image %d is empty (%d x %d)", i, b, hs[e], ws[e]);
            CSEG_REQUIRE((long)hs[e] * ws[e] < 2147483647L, "ms_fuse_argmax_ragged: term %d of image %d is too large (%d x %d)", i, b,
                         hs[e], ws[e]);
        }
    }
    MsPermuted<RgArgs> P;
    if (perm) {
        int at = 0, val = 0;
        const char* fault = ms_perm_fault(perm, K, &at, &val);
        CSEG_REQUIRE(!fault, "ms_fuse_argmax_ragged: perm[%d] = %d %s (perm must be a permutation of the %d classes)", at, val, fault,
                     K);
        bool any_flipped = false;
        for (int e = 0; flipped && e < n_images * n_terms; ++e) any_flipped = any_flipped || flipped[e];
        CSEG_REQUIRE(any_flipped,
                     "ms_fuse_argmax_ragged: a channel permutation was given but no term has a flipped map to apply it to");
        P.perm.fill(perm, K);
    }
    long pix0 = 0;
    for (int first = 0; first < n_images; first += RG_IMAGES) {
        RgArgs& A = P;
        A.n_images = n_images - first < RG_IMAGES ? n_images - first : RG_IMAGES;
        A.n = n_terms;
        A.K = K;
        long blocks = 0;
        for (int j = 0; j < RG_IMAGES; ++j) {
            RgImage& I = A.im[j];
            I.pix0 = 0; I.W = 1; I.w = 1; I.npix = 0; I.block0 = 0;
            const int b = first + j;
            const bool live = j < A.n_images;
            if (live) {
                const int Wp = geometry[4 * b + 1], h = geometry[4 * b + 2], w = geometry[4 * b + 3];
                I.pix0 = pix0; I.W = Wp; I.w = w; I.npix = h * w; I.block0 = (int)blocks;
                pix0 += I.npix;
                blocks += (I.npix + 255) / 256;
            }
            for (int i = 0; i < MS_MAX_TERMS; ++i) {
                MsTerm& t = A.t[j][i];
                t.a = nullptr; t.b = nullptr; t.h = 1; t.w = 1; t.sy = 0.f; t.sx = 0.f; t.wt = 0.f;
                if (!live || i >= n_terms) continue;
                const int e = b * n_terms + i;
                t.a = plain[e];
                t.b = flipped ? flipped[e] : nullptr;
                t.h = hs[e]; t.w = ws[e];
                t.sy = ac_scale(hs[e], geometry[4 * b]); t.sx = ac_scale(ws[e], geometry[4 * b + 1]);
                t.wt = weights[e];
            }
        }
#define LAUNCH(NT, ARGS) \
    hipLaunchKernelGGL((ms_fuse_kernel<NT, std::decay<decltype(ARGS)>::type>), dim3((unsigned)blocks), dim3(256), 0, stream, ARGS, pred, fused)
#define LAUNCH_BY_TERMS(ARGS)                   \
    do {                                        \
        if (n_terms <= 1) LAUNCH(1, ARGS);      \
        else if (n_terms <= 2) LAUNCH(2, ARGS); \
        else if (n_terms <= 4) LAUNCH(4, ARGS); \
        else LAUNCH(8, ARGS);                   \
    } while (0)
        if (perm) LAUNCH_BY_TERMS(P);
        else LAUNCH_BY_TERMS(A);
#undef LAUNCH_BY_TERMS
#undef LAUNCH
        CSEG_CHECK_LAUNCH("ms_fuse_kernel (ragged)");
    }
    return 1;
}

extern "C" int cseg_ms_fuse_argmax_ragged(int n_images, int n_terms, const float* const* plain, const float* const* flipped,
                                          const int* hs, const int* ws, const float* weights, const int* geometry, int K,
                                          uint8_t* pred, float* fused, cseg_stream_t stream_) {
    return cseg_ms_fuse_argmax_ragged_perm(n_images, n_terms, plain, flipped, hs, ws, weights, nullptr, geometry, K, pred, fused,
                                           stream_);
}
