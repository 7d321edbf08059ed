// spv_infer.hip -- the end of an inference / validation batch as ONE launch: logits -> predictions and running metrics on the device.
//
// Why: a validation loop issues argmax, ==, sum, the cross-entropy kernel, a multiply and two accumulates per batch, each at its
// launch floor, and a captured forward (spectre_vit.inference.InferenceSession) needs its metrics inside the graph.  Nothing here is
// bandwidth work: 512 x 100 fp32 logits are 205 KB, so the kernel is one wave per row and a fixed-order join.
//
//   pred[r]  = index of the first maximum of z_r                          (torch.argmax's documented tie rule)
//   counted  : r < *n_valid and 0 <= y_r < C                               (label -1 = "no label": predicted, never counted)
//   top-k hit: #{j : z_j > z_y} + #{j < y : z_j == z_y} < k                (k = 1: exactly pred == y; no sort)
//   loss_r   = logsumexp(z_r) - z_r[y_r], max-subtracted, fp32             (spv_head.hip's cross entropy, per row)
//   stats   += (seen, top1, topk) as int64 and sum_r loss_r as float64, joined in a fixed order: the same inputs give the same bits
#include "spv_common.h"

namespace {

constexpr int ET = 512;            // threads per workgroup
constexpr int EW = ET / 64;        // waves (= rows in flight) per workgroup
constexpr int E_MAX_WG = 64;       // workgroups: one lane of the folding wave each
constexpr int E_ACC = 4;           // seen, top1, topk, loss_sum
constexpr int E_COUNTER = E_ACC;   // word of the arrival counter
constexpr int E_PART = E_ACC + 1;  // first word of the per-workgroup partials [E_MAX_WG][E_ACC]
constexpr int E_WORDS = E_PART + E_MAX_WG * E_ACC;

__device__ __forceinline__ long long d2w(double v) { return __double_as_longlong(v); }
__device__ __forceinline__ double w2d(long long v) { return __longlong_as_double(v); }

// KJ > 0: lane l keeps classes l, l + 64, ... of its row in registers (every load in flight at once, C <= 64 * KJ);
// KJ == 0: any C, the row is walked three times (the second and third walks hit the cache: a row is at most a few KB)
template <typename T, int KJ>
__global__ __launch_bounds__(ET) void eval_head_kernel(const T* __restrict__ z, const int64_t* __restrict__ labels,
                                                       const int* __restrict__ n_valid, int64_t* __restrict__ pred,
                                                       long long* __restrict__ stats, int rows, int C, int k) {
    __shared__ long long wsum[EW][E_ACC];
    __shared__ long long fold[E_MAX_WG][E_ACC];
    __shared__ bool last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nv = min(max(*n_valid, 0), rows);
    long long seen = 0, top1 = 0, topk = 0;
    double loss = 0.0;
    for (int r = blockIdx.x * EW + wave; r < rows; r += gridDim.x * EW) {
        const T* zr = z + (size_t)r * C;
        const int64_t y = labels[r];
        const bool counted = r < nv && y >= 0 && y < C;
        const float zy = io<T>::ld(zr + (counted ? (int)y : 0));   // clamped, unconditional (one address per wave)
        constexpr int NR = KJ > 0 ? KJ : 1;
        float v[NR];
        if constexpr (KJ > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j) v[j] = io<T>::ld(zr + min(lane + 64 * j, C - 1));
        }
        // first maximum: a lane walks its classes in ascending order and keeps the first of its largest
        float m = -INFINITY;
        int am = C;
        if constexpr (KJ > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int c = lane + 64 * j;
                if (c < C && v[j] > m) { m = v[j]; am = c; }
            }
        } else {
            for (int c = lane; c < C; c += 64) {
                const float x = io<T>::ld(zr + c);
                if (x > m) { m = x; am = c; }
            }
        }
        const float wm = wave_max(m);
        // the smallest index among the lanes that hold the maximum (indices are below 2^24: exact as floats)
        int first = (int)(-wave_max(-(float)((m == wm && am < C) ? am : C)));
        if (first >= C) first = 0;   // a row without an ordered maximum (every entry NaN)
        float s = 0.0f, cnt = 0.0f;
        if constexpr (KJ > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int c = lane + 64 * j;
                if (c < C) {
                    s += expf(v[j] - wm);
                    cnt += (v[j] > zy || (v[j] == zy && c < y)) ? 1.0f : 0.0f;
                }
            }
        } else {
            for (int c = lane; c < C; c += 64) {
                const float x = io<T>::ld(zr + c);
                s += expf(x - wm);
                cnt += (x > zy || (x == zy && c < y)) ? 1.0f : 0.0f;
            }
        }
        const float l = wm + logf(wave_sum(s)) - zy;
        const int above = (int)wave_sum(cnt);   // at most C < 2^24 ones: exact
        if (lane == 0) {
            pred[r] = first;
            if (counted) {
                seen += 1;
                top1 += first == (int)y ? 1 : 0;
                topk += above < k ? 1 : 0;
                loss += (double)l;   // this wave's rows in ascending order
            }
        }
    }
    if (lane == 0) {
        wsum[wave][0] = seen;
        wsum[wave][1] = top1;
        wsum[wave][2] = topk;
        wsum[wave][3] = d2w(loss);
    }
    __syncthreads();
    if (tid == 0) {
        long long a0 = 0, a1 = 0, a2 = 0;
        double a3 = 0.0;
        for (int w = 0; w < EW; ++w) {
            a0 += wsum[w][0];
            a1 += wsum[w][1];
            a2 += wsum[w][2];
            a3 += w2d(wsum[w][3]);
        }
        long long* part = stats + E_PART + (size_t)blockIdx.x * E_ACC;
        part[0] = a0;
        part[1] = a1;
        part[2] = a2;
        part[3] = d2w(a3);
        __threadfence();
        last = atomicAdd(reinterpret_cast<unsigned*>(stats + E_COUNTER), 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last) {
        // the last workgroup to arrive joins the partials in workgroup order (spv_cross_entropy_fwd's scheme) and re-arms the counter
        __threadfence();
        if (tid < (int)gridDim.x * E_ACC) fold[tid / E_ACC][tid % E_ACC] = __builtin_nontemporal_load(stats + E_PART + tid);
        __syncthreads();
        if (tid == 0) {
            long long a0 = stats[0], a1 = stats[1], a2 = stats[2];
            double a3 = 0.0;
            for (int g = 0; g < (int)gridDim.x; ++g) {
                a0 += fold[g][0];
                a1 += fold[g][1];
                a2 += fold[g][2];
                a3 += w2d(fold[g][3]);
            }
            stats[0] = a0;
            stats[1] = a1;
            stats[2] = a2;
            stats[3] = d2w(w2d(stats[3]) + a3);   // the batch's sum, then the running sum: one float64 add per batch
            *reinterpret_cast<unsigned*>(stats + E_COUNTER) = 0u;
        }
    }
}

template <typename T>
void launch_eval_head(const void* logits, const int64_t* labels, const int* n_valid, int64_t* pred, void* stats, int rows, int classes, int k,
                      hipStream_t st) {
    const dim3 grid(std::min(cdiv(rows, EW), E_MAX_WG));
    const T* z = static_cast<const T*>(logits);
    long long* sw = static_cast<long long*>(stats);
    if (classes <= 128)
        hipLaunchKernelGGL((eval_head_kernel<T, 2>), grid, dim3(ET), 0, st, z, labels, n_valid, pred, sw, rows, classes, k);
    else if (classes <= 512)
        hipLaunchKernelGGL((eval_head_kernel<T, 8>), grid, dim3(ET), 0, st, z, labels, n_valid, pred, sw, rows, classes, k);
    else
        hipLaunchKernelGGL((eval_head_kernel<T, 0>), grid, dim3(ET), 0, st, z, labels, n_valid, pred, sw, rows, classes, k);
}

}  // namespace

static_assert(ET >= E_MAX_WG * E_ACC, "one thread per partial word in the fold");

extern "C" int64_t spv_eval_head_stats_words(void) { return E_WORDS; }

extern "C" int spv_eval_head(const void* logits, const int64_t* labels, const int* n_valid, int64_t* pred, void* stats, int rows, int classes,
                             int k, int dtype, void* stream) {
    SPV_CHECK(rows > 0 && classes > 0 && classes < (1 << 24), "spv_eval_head: rows=%d classes=%d", rows, classes);
    SPV_CHECK(k >= 1 && k <= 8, "spv_eval_head: k=%d outside 1..8", k);
    SPV_CHECK(logits && labels && n_valid && pred && stats, "spv_eval_head: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == SPV_F32)
        launch_eval_head<float>(logits, labels, n_valid, pred, stats, rows, classes, k, st);
    else if (dtype == SPV_BF16)
        launch_eval_head<bf16_t>(logits, labels, n_valid, pred, stats, rows, classes, k, st);
    else
        return spv_set_error("spv_eval_head: bad dtype %d", dtype);
    SPV_LAUNCH_CHECK("spv_eval_head");
    return 0;
}
