// Test phase: the pixel-level Cityscapes evaluation (IoU and instance-weighted iIoU per class and category) on the device.
// Reference: lib/metrics/cityscapes_evaluator.py:559-662 (evaluatePair). Per image it adds every pixel to a 34 x 34 matrix
// conf[ground truth][prediction] over raw label ids (no ignore value), then walks np.unique(instance ids > 1000) in ascending order
// and, per instance of a label that is evaluated, builds a full-image mask for its size, its true positives (prediction == label) and
// its category true positives (prediction in the label's category), and adds  tp * (avgClassSize / size)  and
// (size - tp) * (avgClassSize / size)  to running float64 sums per class and per category. Two kernels do the same:
//
// cs_eval_update_kernel   one pass over the unpadded region of every image of a batch. blockIdx.y is the image, the pixels of its
//                  region are walked in region-linear order (row after row, no padding in between) with a grid stride, every lane
//                  of a wave taking part in every round. Matrix: per-block LDS bins (34 * 34 u32), non-zero bins flushed with one
//                  64-bit global atomic each, as confusion_lds_kernel. Instances: a per-image table [10 labels 24..33][1000 instance
//                  numbers][size, tp, catTp] of u32 counters. The pixels of one instance are neighbours, so a wave first merges runs of
//                  equal keys -- head flags from __shfl_up, a segmented inclusive scan of the three counts packed into one int
//                  (8 bits each: a wave holds at most 64) -- and the last lane of a run issues the atomics; waves without an instance
//                  pixel skip the scan. Integer atomics only: exact and order-independent.
//                  Status words (u32, zero = clean; otherwise 0xFFFFFFFF - the smallest flat index b*H*W + y*W + x of an offending
//                  pixel, kept with atomicMax): [0] a ground-truth id above 33, [1] an instance id above 1000 whose label id / 1000 is
//                  outside 24..33, [2] a predicted label id above 33, [3] = 1: a record that does not lie inside the image.
//                  Offending pixels are counted nowhere they would index out of bounds.
// cs_eval_reduce_kernel   ten chains -- the eight evaluated instance classes (24 25 26 27 28 31 32 33; 29 caravan and 30 trailer are
//                  ignoreInEval and skipped entirely) and the categories human {24, 25} and vehicle {26 27 28 31 32 33} -- one wave
//                  each. A chain walks images in batch order, its labels ascending, instance numbers ascending (np.unique's order of
//                  label * 1000 + number): the 64 lanes load 64 slots at a time, the non-empty ones are compacted through LDS with a
//                  prefix scan, and every lane then runs the same sequential float64 accumulation over the compacted list with the
//                  reference's operations, each rounded on its own (no fma). Sums are read from and written back to a device buffer
//                  that persists across calls: one call per batch is the reference's loop over all images.
#include "cseg_common.h"

namespace {

constexpr int CS_L = 34;                 // label ids 0..33
constexpr int CS_FIRST = 24;             // first label with instances
constexpr int CS_NLAB = 10;              // labels 24..33
constexpr int CS_SLOTS = 1000;           // instance number = id % 1000
constexpr int CS_CHAINS = 10;

// avgClassSize of the reference's CArgs (lib/metrics/cityscapes_evaluator.py:70-81), by label id - 24
__device__ const double cs_avg_class_size[CS_NLAB] = {
    3462.4756337644,  /* person */ 3930.4788056518,  /* rider */ 12794.0202738185,  /* car */ 27855.1264367816,  /* truck */
    35732.1511111111, /* bus */ 36771.8241758242, /* caravan */ 16926.9763313609,  /* trailer */ 67583.7075812274,  /* train */
    6298.7200839748,  /* motorcycle */ 4672.3249222261 /* bicycle */};
// chain -> first label index (label id - 24), number of label indices; class chains then category chains
__device__ const int cs_chain_labels[CS_CHAINS][6] = {{0}, {1}, {2}, {3}, {4}, {7}, {8}, {9}, {0, 1}, {2, 3, 4, 7, 8, 9}};
__device__ const int cs_chain_count[CS_CHAINS] = {1, 1, 1, 1, 1, 1, 1, 1, 2, 6};

__device__ __forceinline__ double d_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double d_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}

// records [B][4] i32: x0, y0, bw, bh
__global__ __launch_bounds__(256) void cs_eval_update_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ lut,
                                                             const uint8_t* __restrict__ gt, const uint16_t* __restrict__ inst,
                                                             const int* __restrict__ records, int H, int W,
                                                             unsigned long long* __restrict__ conf, unsigned* __restrict__ table,
                                                             unsigned* __restrict__ status) {
    __shared__ unsigned cs_hist[CS_L * CS_L];
    const int b = blockIdx.y;
    const int x0 = records[4 * b + 0], y0 = records[4 * b + 1], bw = records[4 * b + 2], bh = records[4 * b + 3];
    if (x0 < 0 || y0 < 0 || bw < 0 || bh < 0 || x0 > W - bw || y0 > H - bh) {      // block-uniform: nothing is read
        if (threadIdx.x == 0) atomicMax(&status[3], 1u);
        return;
    }
    for (int e = threadIdx.x; e < CS_L * CS_L; e += 256) cs_hist[e] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long n = (long)bw * bh;
    const long step = (long)gridDim.x * 256;
    const long rounds = (n + step - 1) / step;
    const size_t plane = (size_t)b * H * W;
    unsigned* __restrict__ tab = table + (size_t)b * CS_NLAB * CS_SLOTS * 3;
    for (long r = 0; r < rounds; ++r) {
        const long i = r * step + (long)blockIdx.x * 256 + threadIdx.x;
        int key = -1, packed = 0;
        if (i < n) {
            const int y = (int)(i / bw), x = (int)(i - (long)y * bw);
            const size_t at = plane + (size_t)(y0 + y) * W + (x0 + x);
            const unsigned mark = 0xFFFFFFFFu - (unsigned)at;
            const int g = gt[at];
            const int p = lut[pred[at]];
            const int id = inst[at];
            if (p >= CS_L) atomicMax(&status[2], mark);
            if (g >= CS_L) atomicMax(&status[0], mark);
            if (g < CS_L && p < CS_L) atomicAdd(&cs_hist[g * CS_L + p], 1u);
            if (id > 1000) {
                const int lab = id / 1000;
                if (lab < CS_FIRST || lab >= CS_L) {
                    atomicMax(&status[1], mark);
                } else {
                    key = (lab - CS_FIRST) * CS_SLOTS + (id - lab * 1000);
                    const int cat = lab <= 25 ? (p == 24 || p == 25) : (p >= 26 && p <= 33);
                    packed = 1 | ((p == lab) << 8) | (cat << 16);
                }
            }
        }
        if (wave_sum_i(key >= 0 ? 1 : 0) == 0) continue;        // wave-uniform
        // segmented inclusive scan of the packed counts over runs of equal keys
        const int prev = __shfl_up(key, 1, 64);
        int head = (lane == 0 || prev != key) ? 1 : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int c_o = __shfl_up(packed, o, 64);
            const int h_o = __shfl_up(head, o, 64);
            if (lane >= o && !head) { packed += c_o; head = h_o; }
        }
        const int next = __shfl(key, (lane + 1) & 63, 64);
        if ((lane == 63 || next != key) && key >= 0) {
            unsigned* slot = tab + 3 * key;
            atomicAdd(&slot[0], (unsigned)(packed & 255));
            if ((packed >> 8) & 255) atomicAdd(&slot[1], (unsigned)((packed >> 8) & 255));
            if ((packed >> 16) & 255) atomicAdd(&slot[2], (unsigned)((packed >> 16) & 255));
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < CS_L * CS_L; e += 256) {
        const unsigned c = cs_hist[e];
        if (c) atomicAdd(&conf[e], (unsigned long long)c);
    }
}

// one wave per chain; stats_i [10][2] i64 {tp, fn}, stats_f [10][2] f64 {tpWeighted, fnWeighted}
__global__ __launch_bounds__(64) void cs_eval_reduce_kernel(const unsigned* __restrict__ table, int B, long long* __restrict__ stats_i,
                                                            double* __restrict__ stats_f) {
    __shared__ unsigned cs_list[64][2];
    const int chain = blockIdx.x, lane = threadIdx.x;
    const int field = chain < 8 ? 1 : 2;                    // tp of the class, catTp of the category
    long long tp_sum = stats_i[2 * chain], fn_sum = stats_i[2 * chain + 1];
    double tp_w = stats_f[2 * chain], fn_w = stats_f[2 * chain + 1];
    for (int b = 0; b < B; ++b) {
        for (int l = 0; l < cs_chain_count[chain]; ++l) {
            const int li = cs_chain_labels[chain][l];
            const double avg = cs_avg_class_size[li];
            const unsigned* __restrict__ row = table + ((size_t)b * CS_NLAB + li) * CS_SLOTS * 3;
            unsigned sizes[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int s = c * 64 + lane;
                sizes[c] = s < CS_SLOTS ? row[3 * s] : 0u;
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int nz = sizes[c] ? 1 : 0;
                const int incl = wave_incl_scan_i(nz, lane);
                const int total = __shfl(incl, 63, 64);
                if (total == 0) continue;                   // wave-uniform
                if (nz) {
                    cs_list[incl - 1][0] = sizes[c];
                    cs_list[incl - 1][1] = row[3 * (c * 64 + lane) + field];
                }
                CSEG_WAVE_LOCKSTEP();
                for (int k = 0; k < total; ++k) {           // every lane runs the same chain on the same values
                    const unsigned size = cs_list[k][0], tp = cs_list[k][1];
                    const double weight = avg / (double)size;
                    tp_sum += tp;
                    fn_sum += size - tp;
                    tp_w = d_add(tp_w, d_mul((double)tp, weight));
                    fn_w = d_add(fn_w, d_mul((double)(size - tp), weight));
                }
                CSEG_WAVE_LOCKSTEP();                       // the list is rewritten by the next non-empty chunk
            }
        }
    }
    if (lane == 0) {
        stats_i[2 * chain] = tp_sum;
        stats_i[2 * chain + 1] = fn_sum;
        stats_f[2 * chain] = tp_w;
        stats_f[2 * chain + 1] = fn_w;
    }
}

}  // namespace

extern "C" int cseg_cs_eval_update(const uint8_t* pred, const uint8_t* lut, const uint8_t* labelmap_raw, const uint16_t* instancemap,
                                   const int32_t* records_host, const int32_t* records, int B, int H, int W, int64_t* conf,
                                   uint32_t* table, uint32_t* status, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(B >= 0 && B <= 65535, "cs_eval_update: B = %d images (at most 65535 are supported)", B);
    CSEG_REQUIRE(H > 0 && W > 0, "cs_eval_update: H = %d, W = %d", H, W);
    CSEG_REQUIRE((long)B * H * W < 2147483648L, "cs_eval_update: %ld pixels in one call (fewer than 2^31 are supported)", (long)B * H * W);
    if (B == 0) return 1;
    CSEG_REQUIRE(pred && lut && labelmap_raw && instancemap && records_host && records && conf && table && status,
                 "cs_eval_update: null pointer");
    long most = 0;
    for (int b = 0; b < B; ++b) {
        const int x0 = records_host[4 * b], y0 = records_host[4 * b + 1], bw = records_host[4 * b + 2], bh = records_host[4 * b + 3];
        CSEG_REQUIRE(x0 >= 0 && y0 >= 0 && bw >= 0 && bh >= 0 && x0 <= W - bw && y0 <= H - bh,
                     "cs_eval_update: records[%d] = (x0 %d, y0 %d, bw %d, bh %d) does not lie inside the %d x %d image", b, x0, y0, bw, bh,
                     H, W);
        most = (long)bw * bh > most ? (long)bw * bh : most;
    }
    if (most == 0) return 1;
    // 16 pixels per thread and at most 256 blocks per image: a block's flush of its LDS bins is amortised over >= 4096 pixels
    const long want = (most + 256L * 16 - 1) / (256L * 16);
    const unsigned blocks = (unsigned)(want > 256 ? 256 : want);
    hipLaunchKernelGGL(cs_eval_update_kernel, dim3(blocks, (unsigned)B), dim3(256), 0, stream, pred, lut, labelmap_raw, instancemap, records,
                       H, W, reinterpret_cast<unsigned long long*>(conf), table, status);
    CSEG_CHECK_LAUNCH("cs_eval_update_kernel");
    return 1;
}

extern "C" int cseg_cs_eval_reduce(const uint32_t* table, int B, int64_t* stats_i, double* stats_f, cseg_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CSEG_REQUIRE(B >= 0, "cs_eval_reduce: B = %d", B);
    if (B == 0) return 1;
    CSEG_REQUIRE(table && stats_i && stats_f, "cs_eval_reduce: null pointer");
    hipLaunchKernelGGL(cs_eval_reduce_kernel, dim3(CS_CHAINS), dim3(64), 0, stream, table, B, reinterpret_cast<long long*>(stats_i),
                       stats_f);
    CSEG_CHECK_LAUNCH("cs_eval_reduce_kernel");
    return 1;
}
