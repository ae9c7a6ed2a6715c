// cv2's INTER_CUBIC coefficient arithmetic for 8-bit images, shared by augment.hip and augment_ragged.hip: the float operations of
// interpolateCubic spelled one rounding at a time, and the Q11 coefficient table of one destination coordinate. cubic_eval.hip takes
// the same operations, and the float coefficients of cv2's float images (cubic_coeffs_f32), from here.
#pragma once
#include "cseg_common.h"

namespace {

// Individually rounded float operations. hipcc's default is -ffp-contract=fast, which fuses a product and a sum into one FMA even
// across statements and inlined calls -- ROCm 7.2's own __fmul_rn / __fadd_rn are plain `x * y` / `x + y` and fuse as well
// (checked in the gfx950 assembly) -- so the operations are spelled here under `contract(off)`: they carry no `contract` flag and the
// backend has nothing it may fuse.
__device__ __forceinline__ float f_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float f_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float f_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// OpenCV interpolateCubic (modules/imgproc/src/resize.cpp) in float with the source's operation order, every product and sum rounded
// on its own, then saturate_cast<short>(c * INTER_RESIZE_COEF_SCALE) with INTER_RESIZE_COEF_BITS = 11 (cvRound: half to even).
__device__ __forceinline__ void cubic_coeffs_q11(float t, int (&q)[4]) {
    const float A = -0.75f;
    const float x1 = f_add(t, 1.f);
    float c[4];
    c[0] = f_sub(f_mul(f_add(f_mul(f_sub(f_mul(A, x1), 5.f * A), x1), 8.f * A), x1), 4.f * A);
    c[1] = f_add(f_mul(f_mul(f_sub(f_mul(A + 2.f, t), A + 3.f), t), t), 1.f);
    const float u = f_sub(1.f, t);
    c[2] = f_add(f_mul(f_mul(f_sub(f_mul(A + 2.f, u), A + 3.f), u), u), 1.f);
    c[3] = f_sub(f_sub(f_sub(1.f, c[0]), c[1]), c[2]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float r = rintf(f_mul(c[k], 2048.f));
        q[k] = (int)fminf(fmaxf(r, -32768.f), 32767.f);
    }
}

// The same interpolateCubic for float images (cv2's float INTER_CUBIC keeps the coefficients as they come, no Q11 step): the
// operations and their order are those of cubic_coeffs_q11 above, c[3] = 1 - c[0] - c[1] - c[2] included. cubic_eval.hip.
__device__ __forceinline__ void cubic_coeffs_f32(float t, float (&c)[4]) {
    const float A = -0.75f;
    const float x1 = f_add(t, 1.f);
    c[0] = f_sub(f_mul(f_add(f_mul(f_sub(f_mul(A, x1), 5.f * A), x1), 8.f * A), x1), 4.f * A);
    c[1] = f_add(f_mul(f_mul(f_sub(f_mul(A + 2.f, t), A + 3.f), t), t), 1.f);
    const float u = f_sub(1.f, t);
    c[2] = f_add(f_mul(f_mul(f_sub(f_mul(A + 2.f, u), A + 3.f), u), u), 1.f);
    c[3] = f_sub(f_sub(f_sub(1.f, c[0]), c[1]), c[2]);
}

}  // namespace
