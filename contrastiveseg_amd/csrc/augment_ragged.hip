// GPU data pipeline for mixed-size datasets (COCO-Stuff, ADE20K, Pascal-Context, Mapillary: every reference config with `resize` in
// its transform sequence). augment.hip walks ONE resampling backwards per output pixel and needs a batch of equal-sized sources; here
// every sample has its own size in a packed ("ragged") buffer, and the reference chain may hold TWO resamplings:
//   lib/datasets/tools/cv2_aug_transforms.py:605-651  Resize         cv2.resize INTER_CUBIC .astype(uint8) / INTER_NEAREST
//   lib/datasets/tools/cv2_aug_transforms.py:327-443  RandomResize   the same, on the result
// The intermediate image is rounded to bytes, so the two do not collapse into one (85 % of the pixels of a smooth image differ from a
// direct resize, by up to 24 grey levels). Hence two stages:
//   stage 1  resize_ragged_kernel   runs only for samples with two non-identity resamplings: raw -> intermediate uint8 image and
//                                   uint8 label at the sample's own W1 x H1, into a second packed buffer. The label IS resampled here
//                                   (not composed into stage 2's index map), so stage 2 reads image and label from one source.
//   stage 2  augment_ragged_kernel  the work of augment_kernel (pad -> flip -> crop -> one resize -> brightness -> normalise -> LUT ->
//                                   ReLabel) with a per-sample source: the raw buffer or the stage-1 buffer.
// A horizontal flip AHEAD of a resampling is not a flip after it (cv2's nearest rule min(floor(d * scale), W - 1) and the cubic taps
// are not mirror-symmetric on the pixel grid), so each stage has a `mirror` flag that reads the source columns mirrored -- which
// equals flipping the source first. The host (lib/datasets/tools/gpu_aug.py) walks the sequence in order and folds every flip into
// one of: stage-1 mirror, stage-2 mirror, mirrored crop window, output flip.
// Arithmetic: cseg_cubic.h (the Q11 rule of augment.hip), integer after the float coefficient tables; plain loads and stores, no
// atomics, no LDS: the result cannot depend on the order of waves. Stores: 64 consecutive X per wave into each fp32 plane, as in
// augment.hip. Records and offsets are validated on the HOST copy before any launch (an offset past the buffer is an out-of-bounds
// read on the device).
#include "cseg_common.h"
#include "cseg_cubic.h"

namespace {

struct RaggedDims {
    int B, Ht, Wt;
    float div, mean[3], std[3];
};

struct RaggedSrc {
    const uint8_t* img;      // [H][W][3]
    const uint8_t* lab;      // [H][W] or nullptr
    int W, H;
};

// One pixel (xr, yr) of cv2.resize(mirror ? flip(src) : src, (Wr, Hr)): INTER_CUBIC on the image (v, grey levels 0..255),
// INTER_NEAREST on the label (ls; 255 without labels). Wr x Hr equal to the source size is a copy, as in cv::resize.
__device__ __forceinline__ void resample_pixel(const RaggedSrc& s, int Wr, int Hr, int mirror, int xr, int yr, int (&v)[3], int& ls) {
    if (Wr == s.W && Hr == s.H) {
        const int xs = mirror ? s.W - 1 - xr : xr;
        const uint8_t* q = s.img + ((size_t)yr * s.W + xs) * 3;
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
        ls = s.lab ? s.lab[(size_t)yr * s.W + xs] : 255;
        return;
    }
    // cv::resize: scale = 1 / (dsize / ssize) in double; source coordinate (dst + 0.5) * scale - 0.5
    const double scx = 1.0 / ((double)Wr / (double)s.W), scy = 1.0 / ((double)Hr / (double)s.H);
    const float fx = (float)(((double)xr + 0.5) * scx - 0.5), fy = (float)(((double)yr + 0.5) * scy - 0.5);
    const int sx = (int)floorf(fx), sy = (int)floorf(fy);
    int ax[4], ay[4];
    cubic_coeffs_q11(f_sub(fx, (float)sx), ax);
    cubic_coeffs_q11(f_sub(fy, (float)sy), ay);
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int yy = min(max(sy - 1 + j, 0), s.H - 1);
        const uint8_t* row = s.img + (size_t)yy * s.W * 3;
        int r0 = 0, r1 = 0, r2 = 0;                          // HResizeCubic<uchar, int, short>: one row of the horizontal pass
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xx = min(max(sx - 1 + i, 0), s.W - 1);    // column of the (flipped) image cv2 sees
            const uint8_t* q = row + (size_t)(mirror ? s.W - 1 - xx : xx) * 3;
            r0 += ax[i] * (int)q[0]; r1 += ax[i] * (int)q[1]; r2 += ax[i] * (int)q[2];
        }
        acc[0] += ay[j] * r0; acc[1] += ay[j] * r1; acc[2] += ay[j] * r2;      // VResizeCubic
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)                              // FixedPtCast<int, uchar, 22>: (v + 2^21) >> 22, saturated
        v[c] = min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
    // INTER_NEAREST: min(floor(dst * scale), src - 1)
    const int nx = min((int)floor((double)xr * scx), s.W - 1), ny = min((int)floor((double)yr * scy), s.H - 1);
    ls = s.lab ? s.lab[(size_t)ny * s.W + (mirror ? s.W - 1 - nx : nx)] : 255;
}

__global__ __launch_bounds__(256) void resize_ragged_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                            const int32_t* __restrict__ params, const int64_t* __restrict__ offsets,
                                                            uint8_t* __restrict__ mid_img, uint8_t* __restrict__ mid_lab) {
    const int b = blockIdx.z;
    const int32_t* p = params + (size_t)b * CSEG_AUG_RAGGED_PARAM_INTS;
    const int W1 = p[2], H1 = p[3];
    if ((int)blockIdx.x * 64 >= W1 || (int)blockIdx.y * 4 >= H1) return;       // stage skipped (W1 = 0) or outside this sample
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X >= W1 || Y >= H1) return;
    const int64_t so = offsets[2 * b], mo = offsets[2 * b + 1];
    RaggedSrc s;
    s.img = img + (size_t)so * 3; s.lab = lab ? lab + so : nullptr; s.W = p[0]; s.H = p[1];
    int v[3], ls;
    resample_pixel(s, W1, H1, p[4], X, Y, v, ls);
    uint8_t* o = mid_img + ((size_t)mo + (size_t)Y * W1 + X) * 3;
    o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
    if (mid_lab) mid_lab[(size_t)mo + (size_t)Y * W1 + X] = (uint8_t)ls;
}

__global__ __launch_bounds__(256) void augment_ragged_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ lab,
                                                             const uint8_t* __restrict__ mid_img, const uint8_t* __restrict__ mid_lab,
                                                             const int16_t* __restrict__ lut,
                                                             const int16_t* __restrict__ lut_mirrored,
                                                             const int32_t* __restrict__ params,
                                                             const int64_t* __restrict__ offsets, RaggedDims d,
                                                             float* __restrict__ out_img, int64_t* __restrict__ out_lab) {
    const int b = blockIdx.z;
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), Y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (X >= d.Wt || Y >= d.Ht) return;
    const int32_t* p = params + (size_t)b * CSEG_AUG_RAGGED_PARAM_INTS;
    const int Wr = p[5], Hr = p[6], mirror = p[7], x_off = p[8], y_off = p[9], tw = p[10], th = p[11];
    const int flip = p[12], shift = p[13], left_pad = p[14], up_pad = p[15];
    const size_t plane = (size_t)d.Ht * d.Wt;
    float* o = out_img + (size_t)b * 3 * plane + (size_t)Y * d.Wt + X;
    int64_t* ol = out_lab ? out_lab + (size_t)b * plane + (size_t)Y * d.Wt + X : nullptr;
    const int xc = X - left_pad, yc = Y - up_pad;
    if (xc < 0 || xc >= tw || yc < 0 || yc >= th) {          // collate padding: normalised image 0, label -1
        o[0] = 0.f; o[plane] = 0.f; o[2 * plane] = 0.f;
        if (ol) *ol = -1;
        return;
    }
    const int xr = x_off + (flip ? tw - 1 - xc : xc), yr = y_off + yc;      // pixel of the resized image
    RaggedSrc s;
    if (p[2] > 0) {                                          // two resamplings: stage 1 left its W1 x H1 result in the second buffer
        const int64_t mo = offsets[2 * b + 1];
        s.img = mid_img + (size_t)mo * 3; s.lab = lab ? mid_lab + mo : nullptr; s.W = p[2]; s.H = p[3];
    } else {
        const int64_t so = offsets[2 * b];
        s.img = img + (size_t)so * 3; s.lab = lab ? lab + so : nullptr; s.W = p[0]; s.H = p[1];
    }
    int v[3], ls;
    resample_pixel(s, Wr, Hr, mirror, xr, yr, v, ls);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = fminf(fmaxf((float)v[c] + (float)shift, 0.f), 255.f);   // brightness: integer shift, clip
        o[c * plane] = (t / d.div - d.mean[c]) / d.std[c];
    }
    if (ol) {
        // RandomHFlip.swap_pair: the label is swapped iff the sample went through an odd number of flips -- the two stage mirrors
        // and the output flip (the mirrored crop window leaves the flip pending, so it does not count). Stage 1 keeps raw ids.
        const int16_t* table = (((p[4] ^ mirror ^ flip) & 1) && lut_mirrored) ? lut_mirrored : lut;
        const int t = table ? (int)table[ls] : ls;
        *ol = (t == 255) ? -1 : (int64_t)t;                                    // ReLabel(255, -1)
    }
}

// The host copy of the records and offsets, checked sample by sample: what the kernels index with must stay inside the buffers.
// -> 1, and the largest stage-1 size over the batch (0 x 0: no sample needs stage 1).
int check_records(const char* who, const int32_t* ph, const int64_t* oh, int B, long src_pixels, long mid_pixels, int* maxW1,
                  int* maxH1) {
    *maxW1 = *maxH1 = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t* p = ph + (size_t)b * CSEG_AUG_RAGGED_PARAM_INTS;
        const long W0 = p[0], H0 = p[1], W1 = p[2], H1 = p[3];
        CSEG_REQUIRE(W0 > 0 && H0 > 0, "%s: sample %d has a non-positive source size %ldx%ld", who, b, W0, H0);
        CSEG_REQUIRE(oh[2 * b] >= 0 && oh[2 * b] + W0 * H0 <= src_pixels,
                     "%s: sample %d at offset %ld with %ldx%ld pixels reads past the source buffer of %ld pixels", who, b,
                     (long)oh[2 * b], W0, H0, src_pixels);
        CSEG_REQUIRE((W1 > 0) == (H1 > 0) && W1 >= 0 && H1 >= 0, "%s: sample %d has a bad stage-1 size %ldx%ld", who, b, W1, H1);
        if (W1 > 0) {
            CSEG_REQUIRE(oh[2 * b + 1] >= 0 && oh[2 * b + 1] + W1 * H1 <= mid_pixels,
                         "%s: sample %d at offset %ld with %ldx%ld pixels lies past the stage-1 buffer of %ld pixels", who, b,
                         (long)oh[2 * b + 1], W1, H1, mid_pixels);
            if (W1 > *maxW1) *maxW1 = (int)W1;
            if (H1 > *maxH1) *maxH1 = (int)H1;
        }
        const int Wr = p[5], Hr = p[6], x = p[8], y = p[9], tw = p[10], th = p[11];
        CSEG_REQUIRE(Wr > 0 && Hr > 0, "%s: sample %d has a non-positive resized size %dx%d", who, b, Wr, Hr);
        CSEG_REQUIRE(x >= 0 && y >= 0 && tw >= 0 && th >= 0 && (long)x + tw <= Wr && (long)y + th <= Hr,
                     "%s: sample %d crops %dx%d at (%d, %d) outside its resized image %dx%d", who, b, tw, th, x, y, Wr, Hr);
    }
    return 1;
}

}  // namespace

extern "C" int cseg_resize_ragged(const uint8_t* img, const uint8_t* lab, long src_pixels, const int32_t* params,
                                  const int64_t* offsets, const int32_t* params_host, const int64_t* offsets_host, int B,
                                  uint8_t* mid_img, uint8_t* mid_lab, long mid_pixels, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(img && params && offsets && params_host && offsets_host, "resize_ragged: null pointer");
    CSEG_REQUIRE((lab == nullptr) == (mid_lab == nullptr), "resize_ragged: label input and output must come together");
    CSEG_REQUIRE(B > 0 && B <= 65535, "resize_ragged: B = %d outside 1..65535", B);
    CSEG_REQUIRE(src_pixels > 0 && mid_pixels >= 0, "resize_ragged: bad buffer length");
    int maxW1, maxH1;
    if (!check_records("resize_ragged", params_host, offsets_host, B, src_pixels, mid_pixels, &maxW1, &maxH1)) return 0;
    if (maxW1 == 0) return 1;                                // no sample has two resamplings: nothing to launch
    CSEG_REQUIRE(mid_img, "resize_ragged: null pointer");
    CSEG_REQUIRE((maxH1 + 3) / 4 <= 65535, "resize_ragged: stage-1 height %d too large", maxH1);
    dim3 grid((maxW1 + 63) / 64, (maxH1 + 3) / 4, B);
    hipLaunchKernelGGL(resize_ragged_kernel, grid, dim3(256), 0, stream, img, lab, params, offsets, mid_img, mid_lab);
    CSEG_CHECK_LAUNCH("resize_ragged_kernel");
    return 1;
}

extern "C" int cseg_augment_ragged_swap(const uint8_t* img, const uint8_t* lab, long src_pixels, const uint8_t* mid_img,
                                        const uint8_t* mid_lab, long mid_pixels, const int16_t* lut, const int16_t* lut_mirrored,
                                        const int32_t* params, const int64_t* offsets, const int32_t* params_host,
                                        const int64_t* offsets_host, int B, int Ht, int Wt, float div_value, const float* mean3,
                                        const float* std3, float* out_img, int64_t* out_lab, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(img && params && offsets && params_host && offsets_host && out_img && mean3 && std3, "augment_ragged: null pointer");
    CSEG_REQUIRE((lab == nullptr) == (out_lab == nullptr), "augment_ragged: label input and output must come together");
    CSEG_REQUIRE(B > 0 && B <= 65535, "augment_ragged: B = %d outside 1..65535", B);
    CSEG_REQUIRE(Ht > 0 && Wt > 0 && (Ht + 3) / 4 <= 65535, "augment_ragged: bad output size %dx%d", Wt, Ht);
    CSEG_REQUIRE(src_pixels > 0 && mid_pixels >= 0, "augment_ragged: bad buffer length");
    CSEG_REQUIRE(div_value > 0.f && std3[0] > 0.f && std3[1] > 0.f && std3[2] > 0.f, "augment_ragged: div/std must be > 0");
    int maxW1, maxH1;
    if (!check_records("augment_ragged", params_host, offsets_host, B, src_pixels, mid_pixels, &maxW1, &maxH1)) return 0;
    CSEG_REQUIRE(maxW1 == 0 || (mid_img && (lab == nullptr || mid_lab)), "augment_ragged: a sample reads stage 1 but its buffer is null");
    RaggedDims d;
    d.B = B; d.Ht = Ht; d.Wt = Wt; d.div = div_value;
    for (int c = 0; c < 3; ++c) { d.mean[c] = mean3[c]; d.std[c] = std3[c]; }
    dim3 grid((Wt + 63) / 64, (Ht + 3) / 4, B);
    hipLaunchKernelGGL(augment_ragged_kernel, grid, dim3(256), 0, stream, img, lab, mid_img, mid_lab, lut, lut_mirrored, params, offsets, d,
                       out_img, out_lab);
    CSEG_CHECK_LAUNCH("augment_ragged_kernel");
    return 1;
}

extern "C" int cseg_augment_ragged(const uint8_t* img, const uint8_t* lab, long src_pixels, const uint8_t* mid_img,
                                   const uint8_t* mid_lab, long mid_pixels, const int16_t* lut, const int32_t* params,
                                   const int64_t* offsets, const int32_t* params_host, const int64_t* offsets_host, int B, int Ht,
                                   int Wt, float div_value, const float* mean3, const float* std3, float* out_img, int64_t* out_lab,
                                   cseg_stream_t stream_) {
    return cseg_augment_ragged_swap(img, lab, src_pixels, mid_img, mid_lab, mid_pixels, lut, nullptr, params, offsets, params_host,
                                    offsets_host, B, Ht, Wt, div_value, mean3, std3, out_img, out_lab, stream_);
}
