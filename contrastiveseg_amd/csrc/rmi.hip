// Region mutual information (RMI) segmentation term: lib/loss/rmi_loss.py of the reference (RMILoss.forward_sigmoid ->
// rmi_lower_bound) on the coarse logits, without any [B,K,H,W] tensor. The reference upsamples the logits, builds the one-hot
// labels, a permuted copy and the sigmoid probabilities at label resolution, max-pools both 3 x 3 / 3, stacks nine shifted views
// of each pooled map in float64 and centres them; here the label-resolution values exist only in registers.
//
// Launches (all deterministic: fixed-order block partials, no floating-point atomics):
//   rmi_pool_kernel    thread = one pooled cell of one (image, class): the 3 x 3 window's nine label pixels are interpolated from the
//                      coarse logits with the package's fp32 index arithmetic, each contributes its BCE term, the
//                      window maximum of sigmoid * valid + 1e-6 goes to p_pool (f32), the winning slot to route (u8), "some pixel of
//                      the window carries this class" to l_pool (u8). Padding never wins; the first slot in row-major order wins
//                      among equal maxima (F.max_pool2d).
//   rmi_cov_kernel     block = one (image, class): means of the nine shifted views first, then Cp = p~ p~^T accumulated in float64
//                      from centred values. The label side is 0/1: Cl = N_ij - N_i N_j / M from integer counts (exact up to one
//                      rounding -- raw moments lose nothing there), Clp = sum l_i p~_j (the term -mean(l_i) sum p~_j of the centred
//                      form is zero: centred vectors sum to zero).
//   rmi_solve_kernel   thread = one (image, class), float64, matrices in LDS: both Cholesky factorisations, rmi, d rmi / d Cp and
//                      d rmi / d Clp (derivation in DESIGN.md; the + 1e-8 inside the log is kept by differentiating the factor).
//   rmi_finish_kernel  one block: BCE sum, V, sum of rmi in fixed order -> the loss.
//   rmi_gpool_kernel   thread = one pooled cell: the 9 x 9 stencil that carries the matrix gradients back to p_pool.
//   rmi_bwd_kernel     thread = one coarse logit: the gather adjoint (its own copy of the loop nest) of, per label
//                      pixel, the BCE gradient plus, for the routed pixel of its window, g_pool * sigmoid'.
#include "cseg_taps.h"

namespace {

constexpr double RMI_POS_ALPHA = 1e-3;    // _POS_ALPHA
constexpr double RMI_LOG_EPS = 1e-8;      // inside log_det_by_cholesky
constexpr float RMI_CLIP_MIN = 1e-6f;     // _CLIP_MIN
constexpr int RD = 9;                     // radius * radius
constexpr int RDD = RD * RD;
constexpr int RTRI = RD * (RD + 1) / 2;   // 45
constexpr int SOLVE_T = 16;               // systems per solve block

struct RmiDims {
    int B, K, h, w, H, W, hp, wp;
    float sy, sx;
};

__device__ __forceinline__ float rmi_logit(const float* __restrict__ plane, int w, int y0, int y1, float ly1, int x0, int x1, float lx1) {
    const float ly0 = 1.f - ly1;
    const float r0 = ly0 * plane[(size_t)y0 * w + x0] + ly1 * plane[(size_t)y1 * w + x0];
    const float r1 = ly0 * plane[(size_t)y0 * w + x1] + ly1 * plane[(size_t)y1 * w + x1];
    return fmaf(lx1, r1 - r0, r0);
}

__device__ __forceinline__ float rmi_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------
// pool forward
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rmi_pool_kernel(const float* __restrict__ seg, const int64_t* __restrict__ target, RmiDims d,
                                                       float* __restrict__ p_pool, uint8_t* __restrict__ route,
                                                       uint8_t* __restrict__ l_pool, double* __restrict__ partial) {
    __shared__ double red[2][4];
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const long n_cells = (long)d.B * d.K * d.hp * d.wp;
    double bce = 0.0, nvalid = 0.0;
    if (g < n_cells) {
        const int px = (int)(g % d.wp);
        long r = g / d.wp;
        const int py = (int)(r % d.hp); r /= d.hp;
        const int k = (int)(r % d.K);
        const int b = (int)(r / d.K);
        const float* plane = seg + ((size_t)b * d.K + k) * d.h * d.w;
        const int64_t* tplane = target + (size_t)b * d.H * d.W;
        // max_pool2d drops the last row / column when H / W is a multiple of 3: the last window row / column takes those pixels along
        // for the BCE sum (slot index 3), they are in no window
        const int ny = 3 + ((py == d.hp - 1 && 3 * d.hp - 1 < d.H) ? 1 : 0), nx = 3 + ((px == d.wp - 1 && 3 * d.wp - 1 < d.W) ? 1 : 0);
        int x0[4], x1[4];
        float lx1[4];
#pragma unroll
        for (int dx = 0; dx < 4; ++dx) {
            const int X = min(max(3 * px - 1 + dx, 0), d.W - 1);
            bl_tap(d.sx, d.w, X, x0[dx], x1[dx], lx1[dx]);
        }
        float best = 0.f;
        int slot = -1, lab = 0;
#pragma unroll
        for (int dy = 0; dy < 4; ++dy) {
            const int Y = 3 * py - 1 + dy;
            if (dy >= ny || Y < 0 || Y >= d.H) continue;
            int y0, y1;
            float ly1;
            bl_tap(d.sy, d.h, Y, y0, y1, ly1);
#pragma unroll
            for (int dx = 0; dx < 4; ++dx) {
                const int X = 3 * px - 1 + dx;
                if (dx >= nx || X < 0 || X >= d.W) continue;
                const int64_t t64 = tplane[(size_t)Y * d.W + X];
                const bool valid = t64 >= 0 && t64 < d.K;
                const float x = rmi_logit(plane, d.w, y0, y1, ly1, x0[dx], x1[dx], lx1[dx]);
                float p = RMI_CLIP_MIN;
                if (valid) {
                    const bool hit = t64 == k;
                    lab |= (hit && dy < 3 && dx < 3) ? 1 : 0;
                    bce += (double)(fmaxf(x, 0.f) - (hit ? x : 0.f) + log1pf(expf(-fabsf(x))));
                    if (k == 0) nvalid += 1.0;
                    p = rmi_sigmoid(x) + RMI_CLIP_MIN;
                }
                if (dy < 3 && dx < 3 && (slot < 0 || p > best)) { best = p; slot = dy * 3 + dx; }
            }
        }
        p_pool[g] = best;
        route[g] = (uint8_t)slot;
        l_pool[g] = (uint8_t)lab;
    }
    block_pair_to_partial(wave_sum_d(bce), wave_sum_d(nvalid), red, partial);
}

// ---------------------------------------------------------------------------------------------------------
// covariances: one block per (image, class)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rmi_cov_kernel(const float* __restrict__ p_pool, const uint8_t* __restrict__ l_pool, int hp, int wp,
                                                      double* __restrict__ cov, double* __restrict__ means) {
    __shared__ double red[4][RTRI + RDD + RTRI];
    __shared__ double mp[RD], nl[RD];
    const int bk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* pp = p_pool + (size_t)bk * hp * wp;
    const uint8_t* lp = l_pool + (size_t)bk * hp * wp;
    const int nw = wp - 2, M = (hp - 2) * nw;
    // pass 1: sums of the nine shifted views
    {
        double sp[RD], sl[RD];
#pragma unroll
        for (int i = 0; i < RD; ++i) { sp[i] = 0.0; sl[i] = 0.0; }
        for (int r = tid; r < M; r += 256) {
            const int y = r / nw, x = r - y * nw;
#pragma unroll
            for (int i = 0; i < RD; ++i) {
                const int o = (y + i / 3) * wp + x + i % 3;
                sp[i] += (double)pp[o];
                sl[i] += (double)lp[o];
            }
        }
#pragma unroll
        for (int i = 0; i < RD; ++i) {
            const double a = wave_sum_d(sp[i]), c = wave_sum_d(sl[i]);
            if (lane == 0) { red[wave][i] = a; red[wave][RD + i] = c; }
        }
        __syncthreads();
        if (tid < RD) {
            mp[tid] = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) / (double)M;
            nl[tid] = (red[0][RD + tid] + red[1][RD + tid]) + (red[2][RD + tid] + red[3][RD + tid]);   // a count: exact
        }
        __syncthreads();
    }
    // pass 2: centred p, 0/1 labels
    double cp[RTRI], clp[RDD];
    int nij[RTRI];
#pragma unroll
    for (int i = 0; i < RTRI; ++i) { cp[i] = 0.0; nij[i] = 0; }
#pragma unroll
    for (int i = 0; i < RDD; ++i) clp[i] = 0.0;
    double m[RD];
#pragma unroll
    for (int i = 0; i < RD; ++i) m[i] = mp[i];
    for (int r = tid; r < M; r += 256) {
        const int y = r / nw, x = r - y * nw;
        double pv[RD];
        bool lv[RD];
#pragma unroll
        for (int i = 0; i < RD; ++i) {
            const int o = (y + i / 3) * wp + x + i % 3;
            pv[i] = (double)pp[o] - m[i];
            lv[i] = lp[o] != 0;
        }
        int t = 0;
#pragma unroll
        for (int i = 0; i < RD; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j, ++t) {
                cp[t] += pv[i] * pv[j];
                nij[t] += (lv[i] && lv[j]) ? 1 : 0;
            }
        }
#pragma unroll
        for (int i = 0; i < RD; ++i) {
#pragma unroll
            for (int j = 0; j < RD; ++j) clp[i * RD + j] += lv[i] ? pv[j] : 0.0;
        }
    }
#pragma unroll
    for (int t = 0; t < RTRI; ++t) {
        const double a = wave_sum_d(cp[t]);
        const int c = wave_sum_i(nij[t]);
        if (lane == 0) { red[wave][t] = a; red[wave][RTRI + RDD + t] = (double)c; }
    }
#pragma unroll
    for (int t = 0; t < RDD; ++t) {
        const double a = wave_sum_d(clp[t]);
        if (lane == 0) red[wave][RTRI + t] = a;
    }
    __syncthreads();
    double* out = cov + (size_t)bk * 3 * RDD;       // Cl, Cp, Clp, each 9 x 9 row-major (Clp: rows = label view, columns = p view)
    if (tid < RDD) {
        const int i = tid / RD, j = tid % RD;
        const int hi = max(i, j), lo = min(i, j), t = hi * (hi + 1) / 2 + lo;
        const double n2 = (red[0][RTRI + RDD + t] + red[1][RTRI + RDD + t]) + (red[2][RTRI + RDD + t] + red[3][RTRI + RDD + t]);
        out[tid] = n2 - nl[i] * nl[j] / (double)M;
        out[RDD + tid] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        out[2 * RDD + tid] = (red[0][RTRI + tid] + red[1][RTRI + tid]) + (red[2][RTRI + tid] + red[3][RTRI + tid]);
    }
    if (tid < RD) {
        means[(size_t)bk * 2 * RD + tid] = nl[tid] / (double)M;
        means[(size_t)bk * 2 * RD + RD + tid] = mp[tid];
    }
}

// ---------------------------------------------------------------------------------------------------------
// solve: one (image, class) per thread, float64, five 9 x 9 matrices per thread in LDS (element-major: no bank conflicts)
// ---------------------------------------------------------------------------------------------------------
struct Mat {
    double* p;       // element (i, j) at p[(i * 9 + j) * SOLVE_T]
    __device__ __forceinline__ double& operator()(int i, int j) const { return p[(i * RD + j) * SOLVE_T]; }
};

// in place: lower triangle of a -> its Cholesky factor (the upper triangle is not read; torch.cholesky reads the lower one too)
__device__ void rmi_cholesky(const Mat& a) {
    for (int j = 0; j < RD; ++j) {
        double s = a(j, j);
        for (int k = 0; k < j; ++k) s -= a(j, k) * a(j, k);
        const double ljj = sqrt(s);
        a(j, j) = ljj;
        for (int i = j + 1; i < RD; ++i) {
            double v = a(i, j);
            for (int k = 0; k < j; ++k) v -= a(i, k) * a(j, k);
            a(i, j) = v / ljj;
        }
    }
}

// n = l^-1 (both lower triangular; n's upper triangle is set to zero)
__device__ void rmi_lower_inverse(const Mat& l, const Mat& n) {
    for (int j = 0; j < RD; ++j) {
        for (int i = 0; i < j; ++i) n(i, j) = 0.0;
        n(j, j) = 1.0 / l(j, j);
        for (int i = j + 1; i < RD; ++i) {
            double s = 0.0;
            for (int k = j; k < i; ++k) s -= l(i, k) * n(k, j);
            n(i, j) = s / l(i, i);
        }
    }
}

__global__ __launch_bounds__(SOLVE_T) void rmi_solve_kernel(const double* __restrict__ cov, int n, double* __restrict__ rmi,
                                                            double* __restrict__ grads) {
    __shared__ double sm[5][RDD][SOLVE_T];
    const int tid = threadIdx.x, s = blockIdx.x * SOLVE_T + tid;
    if (s >= n) return;
    const Mat S{&sm[0][0][tid]}, X{&sm[1][0][tid]}, Wm{&sm[2][0][tid]}, Nm{&sm[3][0][tid]}, E{&sm[4][0][tid]};
    const double* cl = cov + (size_t)s * 3 * RDD;
    const double* cpv = cl + RDD;
    const double* clp = cl + 2 * RDD;
    for (int i = 0; i < RD; ++i)
        for (int j = 0; j < RD; ++j) {
            S(i, j) = clp[i * RD + j];
            X(i, j) = cpv[i * RD + j] + (i == j ? RMI_POS_ALPHA : 0.0);
        }
    // (Cp + alpha I)^-1 = N^T N with N the inverse of the Cholesky factor
    rmi_cholesky(X);
    rmi_lower_inverse(X, Nm);
    for (int i = 0; i < RD; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = 0.0;
            for (int k = i; k < RD; ++k) v += Nm(k, i) * Nm(k, j);
            X(i, j) = v;
            X(j, i) = v;
        }
    // W = Clp (Cp + alpha I)^-1
    for (int i = 0; i < RD; ++i)
        for (int j = 0; j < RD; ++j) {
            double v = 0.0;
            for (int k = 0; k < RD; ++k) v += S(i, k) * X(k, j);
            Wm(i, j) = v;
        }
    // A + alpha I = Cl - W Clp^T + alpha I (lower triangle), its factor L, rmi = sum log(L_ii + 1e-8)
    for (int i = 0; i < RD; ++i)
        for (int j = 0; j <= i; ++j) {
            double v = cl[i * RD + j] + (i == j ? RMI_POS_ALPHA : 0.0);
            for (int k = 0; k < RD; ++k) v -= Wm(i, k) * S(j, k);
            X(i, j) = v;
        }
    rmi_cholesky(X);
    double acc = 0.0;
    for (int i = 0; i < RD; ++i) {
        const double lii = X(i, i);
        acc += log(lii + RMI_LOG_EPS);
        E(i, 0) = lii / (lii + RMI_LOG_EPS);      // d log(L_ii + eps) / d log L_ii
    }
    rmi[s] = acc;                                 // 0.5 * 2 * sum
    // G = d rmi / d(A + alpha I) = 1/2 L^-T diag(L_ii / (L_ii + eps)) L^-1 (Cholesky backward of a diagonal cotangent)
    rmi_lower_inverse(X, Nm);
    for (int a = 0; a < RD; ++a)
        for (int c = 0; c <= a; ++c) {
            double v = 0.0;
            for (int i = a; i < RD; ++i) v += Nm(i, a) * E(i, 0) * Nm(i, c);
            X(a, c) = 0.5 * v;
        }
    for (int a = 0; a < RD; ++a)
        for (int c = a + 1; c < RD; ++c) X(a, c) = X(c, a);
    // GW = G W;  d rmi / d Clp = -2 G W;  d rmi / d Cp = W^T G W (written as Gp + Gp^T = 2 W^T G W)
    double* gp2 = grads + (size_t)s * 2 * RDD;
    double* glp = gp2 + RDD;
    for (int i = 0; i < RD; ++i)
        for (int j = 0; j < RD; ++j) {
            double v = 0.0;
            for (int k = 0; k < RD; ++k) v += X(i, k) * Wm(k, j);
            Nm(i, j) = v;
            glp[i * RD + j] = -2.0 * v;
        }
    for (int a = 0; a < RD; ++a)
        for (int c = 0; c < RD; ++c) {
            double v = 0.0;
            for (int i = 0; i < RD; ++i) v += Wm(i, a) * Nm(i, c);
            gp2[a * RD + c] = 2.0 * v;
        }
}

// ---------------------------------------------------------------------------------------------------------
// finish: outd = {loss, bce, rmi_loss, V}, out = (float)loss
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void rmi_finish_kernel(const double* __restrict__ partial, int n_blocks, const double* __restrict__ rmi,
                                                          int B, int K, double c_bce, double c_rmi, double* __restrict__ outd,
                                                          float* __restrict__ out) {
    __shared__ double red[2][16];
    double a = 0.0, v = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += 1024) { a += partial[2 * (size_t)i]; v += partial[2 * (size_t)i + 1]; }
    a = wave_sum_d(a);
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = v; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sv = 0.0;
        for (int i = 0; i < 16; ++i) { sa += red[0][i]; sv += red[1][i]; }
        double sr = 0.0;                           // sum_c mean_b rmi[b, c] / 9
        for (int c = 0; c < K; ++c) {
            double sc = 0.0;
            for (int b = 0; b < B; ++b) sc += rmi[(size_t)b * K + c];
            sr += sc / (double)B;
        }
        sr /= (double)RD;
        const double bce = sa / (sv + 1.0);
        const double loss = c_bce * bce + c_rmi * sr;
        outd[0] = loss; outd[1] = bce; outd[2] = sr; outd[3] = sv;
        out[0] = (float)loss;
    }
}

// ---------------------------------------------------------------------------------------------------------
// pool gradient: g_pool[q] = sum_i sum_j (Gp + Gp^T)[i, j] p~_j[q - o_i] + Glp[j, i] l~_j[q - o_i] over the views i whose point
// q - o_i exists. (The mean subtraction of the centring adds nothing to the gradient: its adjoint subtracts the mean over the points
// of d / d p~_i, which is a combination of sums of centred vectors, and those are zero.)  grid = (cells / 256, B * K)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rmi_gpool_kernel(const float* __restrict__ p_pool, const uint8_t* __restrict__ l_pool,
                                                        const double* __restrict__ means, const double* __restrict__ grads, int hp, int wp,
                                                        double c_rmi_grad, const float* __restrict__ d_loss, float* __restrict__ g_pool) {
    __shared__ double gp2[RDD], glp[RDD], ml[RD], mp[RD];
    const int bk = blockIdx.y, tid = threadIdx.x;
    if (tid < RDD) {
        gp2[tid] = grads[(size_t)bk * 2 * RDD + tid];
        glp[tid] = grads[(size_t)bk * 2 * RDD + RDD + tid];
    }
    if (tid < RD) {
        ml[tid] = means[(size_t)bk * 2 * RD + tid];
        mp[tid] = means[(size_t)bk * 2 * RD + RD + tid];
    }
    __syncthreads();
    const int q = blockIdx.x * 256 + tid;
    if (q >= hp * wp) return;
    const int qy = q / wp, qx = q - qy * wp;
    const float* pp = p_pool + (size_t)bk * hp * wp;
    const uint8_t* lp = l_pool + (size_t)bk * hp * wp;
    double acc = 0.0;
    for (int i = 0; i < RD; ++i) {
        const int ry = qy - i / 3, rx = qx - i % 3;           // the point of view i that reads cell q
        if (ry < 0 || ry >= hp - 2 || rx < 0 || rx >= wp - 2) continue;
#pragma unroll
        for (int j = 0; j < RD; ++j) {
            const int o = (ry + j / 3) * wp + rx + j % 3;
            acc += gp2[i * RD + j] * ((double)pp[o] - mp[j]) + glp[j * RD + i] * ((double)lp[o] - ml[j]);
        }
    }
    g_pool[(size_t)bk * hp * wp + q] = (float)(c_rmi_grad * (double)d_loss[0] * acc);
}

// ---------------------------------------------------------------------------------------------------------
// backward to the coarse logits: exact adjoint of bilinear(align_corners=True) in gather form. grid = (h * w / 256, K, B)
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rmi_bwd_kernel(const float* __restrict__ seg, const int64_t* __restrict__ target,
                                                      const uint8_t* __restrict__ route, const float* __restrict__ g_pool, RmiDims d,
                                                      double c_bce_grad, const double* __restrict__ outd, const float* __restrict__ d_loss,
                                                      float* __restrict__ d_seg) {
    const int k = blockIdx.y, b = blockIdx.z;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= d.h * d.w) return;
    const int ys = e / d.w, xs = e - ys * d.w;
    const float cb = (float)(c_bce_grad * (double)d_loss[0] / (outd[3] + 1.0));
    int y_lo, y_hi, x_lo, x_hi;
    bl_fine_range(d.sy, d.H, ys, ys, y_lo, y_hi);
    bl_fine_range(d.sx, d.W, xs, xs, x_lo, x_hi);
    const float* plane = seg + ((size_t)b * d.K + k) * d.h * d.w;
    const int64_t* tplane = target + (size_t)b * d.H * d.W;
    const size_t pool_base = ((size_t)b * d.K + k) * d.hp * d.wp;
    float acc = 0.f;
    for (int Y = y_lo; Y <= y_hi; ++Y) {
        int y0, y1;
        float ly1;
        bl_tap(d.sy, d.h, Y, y0, y1, ly1);
        const float wy = bl_adjoint_weight(y0, y1, ly1, ys);
        if (wy == 0.f) continue;
        const int py = (Y + 1) / 3, sy3 = (Y + 1) - 3 * py;
        float racc = 0.f;
        for (int X = x_lo; X <= x_hi; ++X) {
            int x0, x1;
            float lx1;
            bl_tap(d.sx, d.w, X, x0, x1, lx1);
            const float wx = bl_adjoint_weight(x0, x1, lx1, xs);
            if (wx == 0.f) continue;
            const int64_t t64 = tplane[(size_t)Y * d.W + X];
            if (t64 < 0 || t64 >= d.K) continue;                  // invalid pixels: p is the constant 1e-6, no BCE term
            const float x = rmi_logit(plane, d.w, y0, y1, ly1, x0, x1, lx1);
            const float sg = rmi_sigmoid(x);
            float gpix = cb * (sg - (t64 == k ? 1.f : 0.f));
            const int px = (X + 1) / 3, slot = sy3 * 3 + (X + 1) - 3 * px;
            const size_t cell = pool_base + (size_t)py * d.wp + px;
            if (py < d.hp && px < d.wp && route[cell] == slot) gpix += g_pool[cell] * sg * (1.f - sg);   // (a dropped last row / column is in no window)
            racc += wx * gpix;
        }
        acc += wy * racc;
    }
    d_seg[(((size_t)b * d.K + k) * d.h + ys) * d.w + xs] = acc;
}

int rmi_dims(RmiDims* d, int B, int K, int h, int w, int H, int W) {
    UpDims u;
    if (!up_dims("rmi", &u, B, K, h, w, H, W)) return 0;
    *d = RmiDims{B, K, h, w, H, W, (H - 1) / 3 + 1, (W - 1) / 3 + 1, u.sy, u.sx};
    CSEG_REQUIRE(d->hp >= 3 && d->wp >= 3, "rmi: the pooled map is %d x %d (labels %d x %d); the 3 x 3 neighbourhood needs at least "
                 "3 x 3 (the reference yields NaN there)", d->hp, d->wp, H, W);
    CSEG_REQUIRE((long)B * K * d->hp * d->wp < 2147483647L && (long)B * K * h * w < 2147483647L, "rmi: tensor too large");
    return 1;
}

void rmi_coefficients(float lam, int lambda_way, float loss_weight, double* c_bce, double* c_rmi) {
    *c_bce = (double)loss_weight * (lambda_way ? (double)lam : 1.0);
    *c_rmi = (double)loss_weight * (lambda_way ? 1.0 - (double)lam : (double)lam);
}

}  // namespace

extern "C" int cseg_rmi_pool_blocks(int B, int K, int H, int W) {
    if (B <= 0 || K <= 0 || H <= 0 || W <= 0) return 0;
    const long cells = (long)B * K * ((H - 1) / 3 + 1) * ((W - 1) / 3 + 1);
    return (int)((cells + 255) / 256);
}

extern "C" int cseg_rmi_pool_fwd(const float* seg, const int64_t* target, int B, int K, int h, int w, int H, int W, int rmi_radius,
                                 int rmi_pool_way, int rmi_pool_size, int rmi_pool_stride, float* p_pool, uint8_t* route,
                                 uint8_t* l_pool, double* partial, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(rmi_radius == 3, "rmi: rmi_radius %d (only 3, the value of the reference's RMI configs, is implemented)", rmi_radius);
    CSEG_REQUIRE(rmi_pool_way == 0, "rmi: rmi_pool_way %d (only 0, max pooling, is implemented)", rmi_pool_way);
    CSEG_REQUIRE(rmi_pool_size == 3 && rmi_pool_stride == 3, "rmi: rmi_pool_size %d / rmi_pool_stride %d (only 3 / 3 is implemented)",
                 rmi_pool_size, rmi_pool_stride);
    RmiDims d;
    if (!rmi_dims(&d, B, K, h, w, H, W)) return 0;
    const int n_blocks = cseg_rmi_pool_blocks(B, K, H, W);
    hipLaunchKernelGGL(rmi_pool_kernel, dim3(n_blocks), dim3(256), 0, stream, seg, target, d, p_pool, route, l_pool, partial);
    CSEG_CHECK_LAUNCH("rmi_pool_kernel");
    return 1;
}

extern "C" int cseg_rmi_cov(const float* p_pool, const uint8_t* l_pool, int B, int K, int hp, int wp, double* cov, double* means,
                            cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(B > 0 && K > 0, "rmi_cov: empty shape");
    CSEG_REQUIRE(hp >= 3 && wp >= 3, "rmi_cov: the pooled map is %d x %d; the 3 x 3 neighbourhood needs at least 3 x 3", hp, wp);
    CSEG_REQUIRE((long)B * K < 2147483647L && (long)hp * wp < 2147483647L, "rmi_cov: tensor too large");
    hipLaunchKernelGGL(rmi_cov_kernel, dim3(B * K), dim3(256), 0, stream, p_pool, l_pool, hp, wp, cov, means);
    CSEG_CHECK_LAUNCH("rmi_cov_kernel");
    return 1;
}

extern "C" int cseg_rmi_solve(const double* cov, int n, double* rmi, double* grads, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(n > 0, "rmi_solve: no systems");
    hipLaunchKernelGGL(rmi_solve_kernel, dim3((n + SOLVE_T - 1) / SOLVE_T), dim3(SOLVE_T), 0, stream, cov, n, rmi, grads);
    CSEG_CHECK_LAUNCH("rmi_solve_kernel");
    return 1;
}

extern "C" int cseg_rmi_finish(const double* partial, int n_blocks, const double* rmi, int B, int K, float lam, int lambda_way,
                               float loss_weight, double* outd, float* out, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(n_blocks > 0 && B > 0 && K > 0, "rmi_finish: empty shape");
    double c_bce, c_rmi;
    rmi_coefficients(lam, lambda_way, loss_weight, &c_bce, &c_rmi);
    hipLaunchKernelGGL(rmi_finish_kernel, dim3(1), dim3(1024), 0, stream, partial, n_blocks, rmi, B, K, c_bce, c_rmi, outd, out);
    CSEG_CHECK_LAUNCH("rmi_finish_kernel");
    return 1;
}

extern "C" int cseg_rmi_bwd(const float* seg, const int64_t* target, const float* p_pool, const uint8_t* route, const uint8_t* l_pool,
                            const double* means, const double* grads, const double* outd, const float* d_loss, int B, int K, int h,
                            int w, int H, int W, float lam, int lambda_way, float loss_weight, float* g_pool, float* d_seg,
                            cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    RmiDims d;
    if (!rmi_dims(&d, B, K, h, w, H, W)) return 0;
    CSEG_REQUIRE(K <= 65535 && B <= 65535, "rmi_bwd: %d classes / %d images exceed the grid", K, B);
    double c_bce, c_rmi;
    rmi_coefficients(lam, lambda_way, loss_weight, &c_bce, &c_rmi);
    const int cells = d.hp * d.wp;
    CSEG_REQUIRE((long)B * K <= 65535, "rmi_bwd: %d x %d (image, class) planes exceed the grid", B, K);
    hipLaunchKernelGGL(rmi_gpool_kernel, dim3((cells + 255) / 256, B * K), dim3(256), 0, stream, p_pool, l_pool, means, grads, d.hp,
                       d.wp, c_rmi / (double)(RD * B), d_loss, g_pool);
    CSEG_CHECK_LAUNCH("rmi_gpool_kernel");
    hipLaunchKernelGGL(rmi_bwd_kernel, dim3((h * w + 255) / 256, K, B), dim3(256), 0, stream, seg, target, route, g_pool, d, c_bce, outd,
                       d_loss, d_seg);
    CSEG_CHECK_LAUNCH("rmi_bwd_kernel");
    return 1;
}
