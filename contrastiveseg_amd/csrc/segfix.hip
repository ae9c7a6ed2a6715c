// Test phase: SegFix refinement of a finished prediction on the device. Reference: scripts/cityscapes/segfix.py:59-95 (shift): every
// pixel's label is replaced by the bilinear blend of the class INDICES around the point its boundary offset points to, rounded half
// to even. The reference normalises the target coordinate as align_corners=True would ((j + ow) / ((w - 1) / 2) - 1) and hands it to
// F.grid_sample with its default align_corners=False, so the sample point is about (j + ow) * w / (w - 1) - 0.5 and almost every
// pixel is a true blend of up to four indices (classes 3 and 7 can give 5). That is reproduced, not repaired. The fp32 order below is
// the one that has the bits of torch's CPU grid_sample:
//
//     sx = fp32(ow * scale) + j                    sy likewise with oh, i
//     gx = sx / fp32((w - 1) / 2) - 1
//     ix = fma(gx + 1, fp32(w / 2), -0.5);         ix = min(max(ix, 0), w - 1)
//     x0 = floor(ix); wx = ix - x0; ex = 1 - wx;   y0, ny, s_y likewise (s_y = 1 - ny)
//     nw = s_y * ex; ne = s_y * wx; sw = ny * ex; se = ny * wx
//     v  = fma(d, se, fma(c, sw, fma(b, ne, a * nw)))      a = x[y0, x0], b = x[y0, x0 + 1], c = x[y0 + 1, x0], d = x[y0 + 1, x0 + 1]
//     out = u8(round_half_even(v))
//
// Every operation but the three fma is a plain fp32 operation rounded on its own (spelled under contract(off): hipcc would fuse
// them otherwise). A tap at x0 + 1 == w or y0 + 1 == h contributes 0; its weight is 0 there anyway.
//
// segfix_shift_kernel<T>   a streaming pass over the whole [B,H,W] canvas; T = float or int8_t is the element type of the offsets
//                  [B,H,W,2] (row offset, column offset; interleaved as scipy's loadmat returns them). blockIdx.y is the image; a
//                  lane takes four consecutive pixels of one row: one 4-byte load of the prediction, two 16-byte (float) or one
//                  8-byte (int8) load of the eight offsets, one packed 4-byte store per output where the rows start aligned
//                  (W % 4 == 0 and aligned bases: a uniform branch), element by element otherwise. The four byte taps are gathers
//                  into the region of the same image (they hit cache: the sample point is a few pixels away). The rule runs on the
//                  image's unpadded region (x0, y0, bw, bh) with h = bh, w = bw: clamping is at the REGION's edge and no tap reads
//                  the padding; outside the region refined = pred. The pixels whose label changed are counted per image: a wave
//                  sum, the four wave sums through LDS, one integer atomic per block.
#include <cmath>

#include "cseg_common.h"

namespace {

__device__ __forceinline__ float sf_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float sf_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sf_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float sf_div(float a, float b) {      // correctly rounded: hipcc's default for fp32 division
#pragma clang fp contract(off)
    return a / b;
}
__device__ __forceinline__ float sf_fma(float a, float b, float c) {
#if defined(__AMDGCN__)
    return __fmaf_rn(a, b, c);
#else
    return std::fma(a, b, c);
#endif
}

// eight consecutive offsets (four pixels) as fp32
__device__ __forceinline__ void sf_load8(const float* __restrict__ p, bool vec, int n, float (&o)[8]) {
    if (vec) {
        const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
        o[0] = lo.x; o[1] = lo.y; o[2] = lo.z; o[3] = lo.w; o[4] = hi.x; o[5] = hi.y; o[6] = hi.z; o[7] = hi.w;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = k < 2 * n ? p[k] : 0.f;
    }
}
__device__ __forceinline__ void sf_load8(const int8_t* __restrict__ p, bool vec, int n, float (&o)[8]) {
    if (vec) {
        const uint2 raw = *reinterpret_cast<const uint2*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[k] = (float)(int8_t)((raw.x >> (8 * k)) & 255u);
            o[4 + k] = (float)(int8_t)((raw.y >> (8 * k)) & 255u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = k < 2 * n ? (float)p[k] : 0.f;
    }
}

// one coordinate of the rule: offset o, own coordinate j, extent w -> the lower tap t0 in [0, w - 1] and the upper weight
__device__ __forceinline__ void sf_coord(float o, float scale, int j, int w, float norm, float half, int& t0, float& hi) {
    const float s = sf_add(sf_mul(o, scale), (float)j);
    const float g = sf_sub(sf_div(s, norm), 1.f);
    float i = sf_fma(sf_add(g, 1.f), half, -0.5f);
    i = fminf(fmaxf(i, 0.f), (float)(w - 1));              // a NaN becomes 0: the tap stays inside whatever the offsets hold
    const float f = floorf(i);
    t0 = (int)f;
    hi = sf_sub(i, f);
}

// records [B][4] i32: x0, y0, bw, bh
template <class T>
__global__ __launch_bounds__(256) void segfix_shift_kernel(const uint8_t* __restrict__ pred, const T* __restrict__ offsets,
                                                           const int* __restrict__ records, float scale,
                                                           const uint8_t* __restrict__ lut, int H, int W, int vec,
                                                           uint8_t* __restrict__ refined, uint8_t* __restrict__ refined_ids,
                                                           int* __restrict__ changed) {
    __shared__ int sf_red[4];
    const int b = blockIdx.y;
    int rx = records[4 * b + 0], ry = records[4 * b + 1], bw = records[4 * b + 2], bh = records[4 * b + 3];
    if (rx < 0 || ry < 0 || bw < 2 || bh < 2 || rx > W - bw || ry > H - bh) bw = bh = 0;      // block-uniform: no region, a plain copy
    const float norm_x = (float)((double)(bw - 1) / 2.0), norm_y = (float)((double)(bh - 1) / 2.0);
    const float half_x = (float)((double)bw / 2.0), half_y = (float)((double)bh / 2.0);
    const int groups = (W + 3) >> 2;                       // groups of four pixels per row
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const size_t plane = (size_t)b * H * W;
    int count = 0;
    if (g < (long)H * groups) {
        const int y = (int)(g / groups), x = (int)(g - (long)y * groups) << 2;
        const int n = W - x < 4 ? W - x : 4;               // pixels of this group
        const size_t at = plane + (size_t)y * W + x;
        const bool wide = vec && n == 4;
        unsigned in4 = 0u;
        if (wide) {
            in4 = *reinterpret_cast<const unsigned*>(pred + at);
        } else {
            for (int k = 0; k < n; ++k) in4 |= (unsigned)pred[at + k] << (8 * k);
        }
        const int i = y - ry;
        const bool row_in = i >= 0 && i < bh;
        unsigned out4 = in4;
        if (row_in && x + n > rx && x < rx + bw) {         // the group touches the region
            float o[8];
            sf_load8(offsets + 2 * at, wide, n, o);
            const uint8_t* __restrict__ reg = pred + plane + (size_t)ry * W + rx;      // the region's pixel (0, 0)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = x + k - rx;
                if (k < n && j >= 0 && j < bw) {
                    int tx, ty;
                    float wx, ny;
                    sf_coord(o[2 * k + 1], scale, j, bw, norm_x, half_x, tx, wx);
                    sf_coord(o[2 * k], scale, i, bh, norm_y, half_y, ty, ny);
                    const float ex = sf_sub(1.f, wx), s_y = sf_sub(1.f, ny);
                    const float nw = sf_mul(s_y, ex), ne = sf_mul(s_y, wx), sw = sf_mul(ny, ex), se = sf_mul(ny, wx);
                    const bool right = tx + 1 < bw, down = ty + 1 < bh;
                    const uint8_t* __restrict__ r0 = reg + (size_t)ty * W + tx;
                    const float a = (float)r0[0];
                    const float bb = right ? (float)r0[1] : 0.f;
                    const float c = down ? (float)r0[W] : 0.f;
                    const float d = (right && down) ? (float)r0[W + 1] : 0.f;
                    const float v = sf_fma(d, se, sf_fma(c, sw, sf_fma(bb, ne, sf_mul(a, nw))));
                    const unsigned q = (unsigned)(int)rintf(v) & 255u;
                    count += q != ((in4 >> (8 * k)) & 255u) ? 1 : 0;
                    out4 = (out4 & ~(255u << (8 * k))) | (q << (8 * k));
                }
            }
        }
        unsigned ids4 = 0u;
        if (refined_ids) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ids4 |= (unsigned)lut[(out4 >> (8 * k)) & 255u] << (8 * k);
        }
        if (wide) {
            *reinterpret_cast<unsigned*>(refined + at) = out4;
            if (refined_ids) *reinterpret_cast<unsigned*>(refined_ids + at) = ids4;
        } else {
            for (int k = 0; k < n; ++k) {
                refined[at + k] = (uint8_t)((out4 >> (8 * k)) & 255u);
                if (refined_ids) refined_ids[at + k] = (uint8_t)((ids4 >> (8 * k)) & 255u);
            }
        }
    }
    count = wave_sum_i(count);                             // every lane of the block takes part
    if ((threadIdx.x & 63) == 0) sf_red[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = (sf_red[0] + sf_red[1]) + (sf_red[2] + sf_red[3]);
        if (total) atomicAdd(&changed[b], total);
    }
}

template <class T>
int segfix_launch(const uint8_t* pred, const T* offsets, const int32_t* records, float scale, const uint8_t* lut, int B, int H, int W,
                  uint8_t* refined, uint8_t* refined_ids, int32_t* changed, hipStream_t stream) {
    const long groups = (long)H * ((W + 3) / 4);
    const long blocks = (groups + 255) / 256;
    // packed accesses need rows that start on a 4-pixel boundary: W % 4 == 0 and bases aligned to the widest access of each array
    const int vec = (W % 4 == 0) && ((uintptr_t)pred % 4 == 0) && ((uintptr_t)refined % 4 == 0) && ((uintptr_t)refined_ids % 4 == 0) &&
                    ((uintptr_t)offsets % (sizeof(T) == 4 ? 16 : 8) == 0);
    hipLaunchKernelGGL(segfix_shift_kernel<T>, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, stream, pred, offsets, records, scale,
                       lut, H, W, vec, refined, refined_ids, changed);
    CSEG_CHECK_LAUNCH("segfix_shift_kernel");
    return 1;
}

}  // namespace

extern "C" int cseg_segfix_shift(const uint8_t* pred, const void* offsets, int offsets_int8, const int32_t* records_host,
                                 const int32_t* records, float scale, const uint8_t* lut, int B, int H, int W, uint8_t* refined,
                                 uint8_t* refined_ids, int32_t* changed, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(B >= 0 && B <= 65535, "segfix_shift: B = %d images (at most 65535 are supported)", B);
    CSEG_REQUIRE(H > 0 && W > 0, "segfix_shift: H = %d, W = %d", H, W);
    CSEG_REQUIRE((long)B * H * W < 2147483648L, "segfix_shift: %ld pixels in one call (fewer than 2^31 are supported)", (long)B * H * W);
    CSEG_REQUIRE(offsets_int8 == 0 || offsets_int8 == 1, "segfix_shift: offsets_int8 = %d (0: fp32 offsets, 1: int8 offsets)",
                 offsets_int8);
    CSEG_REQUIRE(std::isfinite(scale), "segfix_shift: scale = %f is not finite", (double)scale);
    if (B == 0) return 1;
    CSEG_REQUIRE(pred && offsets && records_host && records && refined && changed, "segfix_shift: null pointer");
    CSEG_REQUIRE(lut || !refined_ids, "segfix_shift: refined_ids without a lut");
    CSEG_REQUIRE(refined != pred && refined_ids != pred, "segfix_shift: the refinement is not in place (the taps read pred)");
    for (int b = 0; b < B; ++b) {
        const int x0 = records_host[4 * b], y0 = records_host[4 * b + 1], bw = records_host[4 * b + 2], bh = records_host[4 * b + 3];
        CSEG_REQUIRE(x0 >= 0 && y0 >= 0 && bw >= 0 && bh >= 0 && x0 <= W - bw && y0 <= H - bh,
                     "segfix_shift: records[%d] = (x0 %d, y0 %d, bw %d, bh %d) does not lie inside the %d x %d image", b, x0, y0, bw, bh,
                     H, W);
        CSEG_REQUIRE(bw >= 2 && bh >= 2,
                     "segfix_shift: records[%d] = (x0 %d, y0 %d, bw %d, bh %d): a region needs at least 2 rows and 2 columns (the "
                     "reference divides by (side - 1) / 2)", b, x0, y0, bw, bh);
    }
    if (offsets_int8)
        return segfix_launch(pred, static_cast<const int8_t*>(offsets), records, scale, lut, B, H, W, refined, refined_ids, changed, stream);
    return segfix_launch(pred, static_cast<const float*>(offsets), records, scale, lut, B, H, W, refined, refined_ids, changed, stream);
}
