// spv_misc.hip -- error plumbing + small bandwidth kernels (casts, transposes, GELU, column sums).
#include "spv_common.h"
#include "spv_adamw_core.h"
#include "spv_prologue_core.h"

#include <string.h>

static thread_local char g_err[512] = "";

int spv_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

// dispatch census (test aid): which kernel family served a call -- spv_path_count(SPV_PATH_*)
long long g_spv_path_counts[SPV_PATH_COUNT] = {0};
extern "C" long long spv_path_count(int which) {
    return (which >= 0 && which < SPV_PATH_COUNT) ? g_spv_path_counts[which] : -1;
}

extern "C" int spv_version(void) { return SPV_ABI_VERSION; }
extern "C" const char* spv_last_error(void) { return g_err; }

namespace {

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void cast_kernel(const TI* __restrict__ src, TO* __restrict__ dst, int64_t n) {
    const int64_t n4 = n >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float v[4];
        io<TI>::ld4(src + 4 * i, v);
        io<TO>::st4(dst + 4 * i, v);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        int64_t i = (n4 << 2) + threadIdx.x;
        io<TO>::st(dst + i, io<TI>::ld(src + i));
    }
}

// dst[c][r] = src[map(r)][c], dst leading dimension ld (>= rows, pad zero filled); 64x64 tile through LDS
// (+1 pad), 256 threads.  map(r) = r, or with rg > 0 the grouped row (r / rg) * gs + roff + r % rg
// (token rows of each image minus its CLS row).
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void cast_transpose_kernel(const TI* __restrict__ src, TO* __restrict__ dst, int rows,
                                                             int cols, int ld, int rg, int gs, int roff) {
    __shared__ float tile[64][65];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        int r = r0 + i, c = c0 + tx;
        float v = 0.0f;
        if (r < rows && c < cols) {
            const size_t sr = rg > 0 ? (size_t)(r / rg) * gs + roff + (r % rg) : (size_t)r;
            v = io<TI>::ld(src + sr * cols + c);
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        int c = c0 + i, r = r0 + tx;
        if (c < cols && r < ld) io<TO>::st(dst + (size_t)c * ld + r, tile[tx][i]);
    }
}

// (weight_shadow_tile, the body of the three kernels that cast weights: spv_prologue_core.h)
template <typename TO>
__global__ __launch_bounds__(256) void weight_shadow_kernel(const float* __restrict__ src, TO* __restrict__ plain, TO* __restrict__ tr,
                                                            int rows, int cols, int ld) {
    __shared__ float tile[32][65];
    weight_shadow_tile<TO>(src, plain, tr, rows, cols, ld, blockIdx.x, blockIdx.y, tile);
}

// every weight of the model in ONE launch (8 launches of 4.9 us each per training step otherwise): workgroup b serves tile
// (tile_x[b], tile_y[b]) of tensor tile_tensor[b]
template <typename TO>
__global__ __launch_bounds__(256) void weight_shadow_multi_kernel(const ShadowTensor* __restrict__ tab, const int* __restrict__ tile_tensor,
                                                                  const int* __restrict__ tile_x, const int* __restrict__ tile_y) {
    __shared__ float tile[32][65];
    const ShadowTensor t = tab[tile_tensor[blockIdx.x]];
    weight_shadow_tile<TO>(t.src, static_cast<TO*>(t.plain), static_cast<TO*>(t.tr), t.rows, t.cols, t.ld, tile_x[blockIdx.x],
                           tile_y[blockIdx.x], tile);
}

template <typename T>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        io<T>::st(y + i, gelu_erf(io<T>::ld(x + i)));
}
template <typename T>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                       T* __restrict__ dx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        io<T>::st(dx + i, io<T>::ld(dy + i) * gelu_erf_grad(io<T>::ld(x + i)));
}
template <typename T>
__global__ __launch_bounds__(256) void axpby_kernel(const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ out,
                                                    float a, float b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        io<T>::st(out + i, a * io<T>::ld(x + i) + b * io<T>::ld(y + i));
}

// column sums: block b sums rows b, b+G, ... for all columns into partials[b][n]; second kernel folds.
// column sums, stage 1: grid (column blocks, row slabs).  A 256-thread workgroup is TX column threads (VEC consecutive
// columns each: 16-/8-byte loads) x TY = 256/TX row threads; slab y sums rows y*TY + ty, + gridDim.y*TY, ...; the TY
// partial rows meet in LDS in a fixed order; one fp32 row of partials per slab.  Wide-and-short inputs (512 x 33280,
// the position-embedding gradient) get many column blocks, tall-and-narrow ones (33280 x 512) many slabs.
template <typename T, int VEC>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ x, float* __restrict__ partials, int rows,
                                                             int n, int tx_log2) {
    __shared__ float red[256 * VEC];
    const int TX = 1 << tx_log2, TY = 256 >> tx_log2;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> tx_log2;
    const int c0 = (blockIdx.x * TX + tx) * VEC;
    float s[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = 0.0f;
    if (c0 < n) {
        const int step = gridDim.y * TY;
        for (int r = blockIdx.y * TY + ty; r < rows; r += step) {
            if constexpr (VEC == 4) {
                float v[4];
                io<T>::ld4(x + (size_t)r * n + c0, v);
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] += v[k];
            } else {
                s[0] += io<T>::ld(x + (size_t)r * n + c0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) red[(ty * TX + tx) * VEC + k] = s[k];
    __syncthreads();
    if (ty == 0 && c0 < n) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            float t = s[k];
            for (int q = 1; q < TY; ++q) t += red[(q * TX + tx) * VEC + k];
            if (c0 + k < n) partials[(size_t)blockIdx.y * n + c0 + k] = t;
        }
    }
}
__global__ __launch_bounds__(256) void colsum_fold_kernel(const float* __restrict__ partials, float* __restrict__ out, int parts,
                                                          int n) {
    // a workgroup owns 32 columns; 8 thread rows split the partial slabs; fixed summation order
    __shared__ float red[8][33];
    const int cx = threadIdx.x & 31, py = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cx;
    float s = 0.0f;
    if (c < n)
        for (int p = py; p < parts; p += 8) s += partials[(size_t)p * n + c];
    red[py][cx] = s;
    __syncthreads();
    if (py == 0 && c < n) {
        float t = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += red[q][cx];
        out[c] = t;
    }
}

inline int ew_blocks(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 2048); }

}  // namespace

extern "C" int spv_cast(const void* src, int sd, void* dst, int dd, int64_t n, void* stream) {
    SPV_CHECK(n >= 0, "spv_cast: n < 0");
    if (n == 0) return 0;
    SPV_CHECK(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "spv_cast: pointers must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int g = ew_blocks((n + 3) / 4);
    if (sd == SPV_F32 && dd == SPV_BF16)
        hipLaunchKernelGGL((cast_kernel<float, bf16_t>), dim3(g), dim3(256), 0, st, (const float*)src, (bf16_t*)dst, n);
    else if (sd == SPV_BF16 && dd == SPV_F32)
        hipLaunchKernelGGL((cast_kernel<bf16_t, float>), dim3(g), dim3(256), 0, st, (const bf16_t*)src, (float*)dst, n);
    else if (sd == SPV_F32 && dd == SPV_F32)
        hipLaunchKernelGGL((cast_kernel<float, float>), dim3(g), dim3(256), 0, st, (const float*)src, (float*)dst, n);
    else if (sd == SPV_BF16 && dd == SPV_BF16)
        hipLaunchKernelGGL((cast_kernel<bf16_t, bf16_t>), dim3(g), dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, n);
    else
        return spv_set_error("spv_cast: bad dtypes %d -> %d", sd, dd);
    SPV_LAUNCH_CHECK("spv_cast");
    return 0;
}

extern "C" int spv_cast_transpose(const void* src, int sd, void* dst, int dd, int rows, int cols, int ld, int rg, int gs,
                                  int roff, void* stream) {
    SPV_CHECK(rows > 0 && cols > 0 && ld >= rows, "spv_cast_transpose: bad shape rows=%d cols=%d ld=%d", rows, cols, ld);
    SPV_CHECK(rg == 0 || (rg > 0 && gs >= rg + roff && roff >= 0), "spv_cast_transpose: bad grouping");
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid(cdiv(cols, 64), cdiv(ld, 64));
    if (sd == SPV_F32 && dd == SPV_BF16)
        hipLaunchKernelGGL((cast_transpose_kernel<float, bf16_t>), grid, dim3(256), 0, st, (const float*)src, (bf16_t*)dst, rows, cols, ld, rg, gs, roff);
    else if (sd == SPV_BF16 && dd == SPV_F32)
        hipLaunchKernelGGL((cast_transpose_kernel<bf16_t, float>), grid, dim3(256), 0, st, (const bf16_t*)src, (float*)dst, rows, cols, ld, rg, gs, roff);
    else if (sd == SPV_F32 && dd == SPV_F32)
        hipLaunchKernelGGL((cast_transpose_kernel<float, float>), grid, dim3(256), 0, st, (const float*)src, (float*)dst, rows, cols, ld, rg, gs, roff);
    else if (sd == SPV_BF16 && dd == SPV_BF16)
        hipLaunchKernelGGL((cast_transpose_kernel<bf16_t, bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)src, (bf16_t*)dst, rows, cols, ld, rg, gs, roff);
    else
        return spv_set_error("spv_cast_transpose: bad dtypes %d -> %d", sd, dd);
    SPV_LAUNCH_CHECK("spv_cast_transpose");
    return 0;
}

extern "C" int spv_weight_shadows_multi(const void* table, const int* tile_tensor, const int* tile_x, const int* tile_y, int ntiles,
                                        int dtype, void* stream) {
    SPV_CHECK(ntiles >= 0, "spv_weight_shadows_multi: ntiles = %d", ntiles);
    if (ntiles == 0) return 0;
    SPV_CHECK(table && tile_tensor && tile_x && tile_y, "spv_weight_shadows_multi: null table");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == SPV_BF16)
        hipLaunchKernelGGL((weight_shadow_multi_kernel<bf16_t>), dim3(ntiles), dim3(256), 0, st, static_cast<const ShadowTensor*>(table),
                           tile_tensor, tile_x, tile_y);
    else if (dtype == SPV_F32)
        hipLaunchKernelGGL((weight_shadow_multi_kernel<float>), dim3(ntiles), dim3(256), 0, st, static_cast<const ShadowTensor*>(table),
                           tile_tensor, tile_x, tile_y);
    else
        return spv_set_error("spv_weight_shadows_multi: bad dtype %d", dtype);
    SPV_LAUNCH_CHECK("spv_weight_shadows_multi");
    return 0;
}

extern "C" int spv_weight_shadows(const float* w, void* plain, void* transposed, int rows, int cols, int ld, int dtype, void* stream) {
    SPV_CHECK(rows > 0 && cols > 0 && ld >= rows, "spv_weight_shadows: bad shape %d x %d, ld %d", rows, cols, ld);
    SPV_CHECK(w != nullptr && transposed != nullptr, "spv_weight_shadows: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid(cdiv(cols, 64), cdiv(ld, 32));
    if (dtype == SPV_BF16)
        hipLaunchKernelGGL((weight_shadow_kernel<bf16_t>), grid, dim3(256), 0, st, w, (bf16_t*)plain, (bf16_t*)transposed, rows, cols, ld);
    else if (dtype == SPV_F32)
        hipLaunchKernelGGL((weight_shadow_kernel<float>), grid, dim3(256), 0, st, w, (float*)plain, (float*)transposed, rows, cols, ld);
    else
        return spv_set_error("spv_weight_shadows: bad dtype %d", dtype);
    SPV_LAUNCH_CHECK("spv_weight_shadows");
    return 0;
}

#define DISPATCH_T(dtype, name, ...)                                        \
    if (dtype == SPV_F32) { using T = float; __VA_ARGS__; }                 \
    else if (dtype == SPV_BF16) { using T = bf16_t; __VA_ARGS__; }          \
    else return spv_set_error("%s: bad dtype %d", name, dtype);

extern "C" int spv_gelu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream) {
    if (n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DISPATCH_T(dtype, "spv_gelu_fwd",
               hipLaunchKernelGGL((gelu_fwd_kernel<T>), dim3(ew_blocks(n)), dim3(256), 0, st, (const T*)x, (T*)y, n));
    SPV_LAUNCH_CHECK("spv_gelu_fwd");
    return 0;
}
extern "C" int spv_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype, void* stream) {
    if (n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DISPATCH_T(dtype, "spv_gelu_bwd",
               hipLaunchKernelGGL((gelu_bwd_kernel<T>), dim3(ew_blocks(n)), dim3(256), 0, st, (const T*)dy, (const T*)x, (T*)dx, n));
    SPV_LAUNCH_CHECK("spv_gelu_bwd");
    return 0;
}
extern "C" int spv_axpby(const void* x, const void* y, void* out, float a, float b, int64_t n, int dtype, void* stream) {
    if (n <= 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DISPATCH_T(dtype, "spv_axpby",
               hipLaunchKernelGGL((axpby_kernel<T>), dim3(ew_blocks(n)), dim3(256), 0, st, (const T*)x, (const T*)y, (T*)out, a, b, n));
    SPV_LAUNCH_CHECK("spv_axpby");
    return 0;
}

// partials: fp32 scratch of >= min(rows,512) * n floats
extern "C" int spv_colsum(const void* x, float* out, float* partials, int rows, int n, int dtype, void* stream) {
    SPV_CHECK(rows > 0 && n > 0, "spv_colsum: empty");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int vec = (n % 4 == 0 && ((uintptr_t)x & 15) == 0) ? 4 : 1;
    const int cthreads = cdiv(n, vec);
    int tx_log2 = 5;  // at least 32 column threads
    while (tx_log2 < 8 && (1 << tx_log2) < cthreads) ++tx_log2;
    const int ty = 256 >> tx_log2;
    const int gx = cdiv(cthreads, 1 << tx_log2);
    // ~1024 workgroups in all, at most 512 slabs (the caller's partial buffer holds min(rows, 512) rows of n floats)
    const int parts = std::max(1, std::min(std::min(cdiv(rows, ty), 512), std::max(1, 1024 / gx)));
    if (vec == 4) {
        DISPATCH_T(dtype, "spv_colsum",
                   hipLaunchKernelGGL((colsum_partial_kernel<T, 4>), dim3(gx, parts), dim3(256), 0, st, (const T*)x, partials, rows, n, tx_log2));
    } else {
        DISPATCH_T(dtype, "spv_colsum",
                   hipLaunchKernelGGL((colsum_partial_kernel<T, 1>), dim3(gx, parts), dim3(256), 0, st, (const T*)x, partials, rows, n, tx_log2));
    }
    SPV_LAUNCH_CHECK("spv_colsum");
    hipLaunchKernelGGL(colsum_fold_kernel, dim3(cdiv(n, 32)), dim3(256), 0, st, partials, out, parts, n);
    SPV_LAUNCH_CHECK("spv_colsum(fold)");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// AdamW over many tensors in ONE launch (the optimizer step the training script drives: torch.optim.AdamW, reference
// spectre_vit/repl/train.py:199-201,237).  torch's fused multi-tensor kernel took 103-117 us per step for the FFT model's
// 63 tensors / 13 MB of parameters (latency bound: most tensors are 512-element LayerNorm vectors); one launch whose
// workgroups are dealt 2048-element chunks from a host-built chunk table streams the same bytes in a few microseconds.
// Arithmetic = torch.optim.AdamW (decoupled weight decay, bias correction, amsgrad off, maximize off).
// The update itself is adamw_chunk (spv_adamw_core.h), shared with the step-control form of the launch (spv_optim.hip).
namespace {
__global__ __launch_bounds__(256) void adamw_multi_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                          const int* __restrict__ chunk_off, const int* __restrict__ sizes, float lr,
                                                          float beta1, float beta2, float omb1, float omb2, float eps, float wd,
                                                          float bc1, float bc2, const float* __restrict__ step_dev) {
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const AdamTensor a = tab[t];
    const int n = sizes[t];
    adamw_chunk<false>(a, n, off, lr, beta1, beta2, omb1, omb2, eps, wd, bc1, bc2, step_dev, 1.0f);
}

// The same launch with the weights' moving average updated from the registers that hold the new weight (spv_adamw_core.h: EMA).
__global__ __launch_bounds__(256) void adamw_multi_ema_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                              const int* __restrict__ chunk_off, const int* __restrict__ sizes, float lr,
                                                              float beta1, float beta2, float omb1, float omb2, float eps, float wd,
                                                              float bc1, float bc2, const float* __restrict__ step_dev,
                                                              float* const* __restrict__ ema_tab, float ema_w, int ema_warmup, float ema_step) {
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const AdamTensor a = tab[t];
    const int n = sizes[t];
    adamw_chunk<false, true>(a, n, off, lr, beta1, beta2, omb1, omb2, eps, wd, bc1, bc2, step_dev, 1.0f, ema_tab[t], ema_w, ema_warmup,
                             ema_step);
}

}  // namespace

extern "C" int spv_adamw_multi(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                               float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                               float bias_correction1, float bias_correction2, const float* step_dev, void* stream) {
    SPV_CHECK(nchunks >= 0, "spv_adamw_multi: nchunks = %d", nchunks);
    if (nchunks == 0) return 0;
    SPV_CHECK(table && chunk_tensor && chunk_off && sizes, "spv_adamw_multi: null table");
    SPV_CHECK(step_dev != nullptr || (bias_correction1 > 0.0f && bias_correction2 > 0.0f), "spv_adamw_multi: bias corrections must be > 0");
    hipLaunchKernelGGL(adamw_multi_kernel, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, lr, beta1, beta2, one_minus_beta1,
                       one_minus_beta2, eps, weight_decay, bias_correction1, bias_correction2, step_dev);
    SPV_LAUNCH_CHECK("spv_adamw_multi");
    return 0;
}

extern "C" int spv_adamw_multi_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                                   float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                                   float bias_correction1, float bias_correction2, const float* step_dev, float* const* ema_table,
                                   float ema_weight, int ema_warmup, float ema_step, void* stream) {
    SPV_CHECK(nchunks >= 0, "spv_adamw_multi_ema: nchunks = %d", nchunks);
    SPV_CHECK(table && chunk_tensor && chunk_off && sizes, "spv_adamw_multi_ema: null table");
    SPV_CHECK(ema_table, "spv_adamw_multi_ema: null ema_table (use spv_adamw_multi for a group that is not averaged)");
    SPV_CHECK(step_dev != nullptr || (bias_correction1 > 0.0f && bias_correction2 > 0.0f), "spv_adamw_multi_ema: bias corrections must be > 0");
    SPV_CHECK(ema_weight > 0.0f && ema_weight <= 1.0f, "spv_adamw_multi_ema: ema_weight = %g must be in (0, 1]", (double)ema_weight);
    SPV_CHECK(!ema_warmup || step_dev != nullptr || ema_step >= 1.0f, "spv_adamw_multi_ema: ema_step = %g must be >= 1 (the step count of this step)",
              (double)ema_step);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(adamw_multi_ema_kernel, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, lr, beta1, beta2, one_minus_beta1,
                       one_minus_beta2, eps, weight_decay, bias_correction1, bias_correction2, step_dev, ema_table, ema_weight, ema_warmup,
                       ema_step);
    SPV_LAUNCH_CHECK("spv_adamw_multi_ema");
    return 0;
}

// ---- device-side seed word for HIP-graph capture (see spv_common.h: g_seed_dev)
int spv_seed_ptr_set_rowops(const unsigned long long* p);
int spv_seed_ptr_set_patch(const unsigned long long* p);
int spv_seed_ptr_set_attn(const unsigned long long* p);
int spv_seed_ptr_set_gemm(const unsigned long long* p);
namespace {
__global__ void seed_advance_kernel(unsigned long long* p) { *p += SEED_STEP; }

// ---- the step prologue: the five launches that open a graph-replayed training step as ONE.  They are mutually independent -- each
// reads only the post-optimizer parameters or the image buffer, and all are needed only in front of the token GEMM -- but as five
// dependent graph nodes of 1 .. 1536 workgroups each paid its own launch and drain.  Workgroup ranges are dealt to the roles in the
// order seed, shadows, fold, patch rows, position rows; a role's workgroup runs the body of its stand-alone kernel with that kernel's
// grid, so every output bit is the stand-alone launch's.
struct PrologueArgs {
    spv_prologue_jobs j;
    int n_seed, n_shadow, n_fold, n_patch, n_pos;   // workgroups per role (0: the role is absent)
    int patch_vec4;
};

__global__ __launch_bounds__(256) void step_prologue_kernel(const PrologueArgs a) {
    __shared__ float tile[32][65];   // the shadows' transpose tile; the other roles use no LDS
    int bid = blockIdx.x;
    if (bid < a.n_seed) {
        if (threadIdx.x == 0) *static_cast<unsigned long long*>(a.j.seed_word) += SEED_STEP;
        return;
    }
    bid -= a.n_seed;
    if (bid < a.n_shadow) {
        const ShadowTensor t = static_cast<const ShadowTensor*>(a.j.shadow_table)[a.j.tile_tensor[bid]];
        if (a.j.shadow_dtype == SPV_BF16)
            weight_shadow_tile<bf16_t>(t.src, static_cast<bf16_t*>(t.plain), static_cast<bf16_t*>(t.tr), t.rows, t.cols, t.ld, a.j.tile_x[bid],
                                       a.j.tile_y[bid], tile);
        else
            weight_shadow_tile<float>(t.src, static_cast<float*>(t.plain), static_cast<float*>(t.tr), t.rows, t.cols, t.ld, a.j.tile_x[bid],
                                      a.j.tile_y[bid], tile);
        return;
    }
    bid -= a.n_shadow;
    if (bid < a.n_fold) {
        spectral_fold_body(a.j.fold_w, a.j.fold_fh, a.j.fold_fw, a.j.fold_out, a.j.fold_embed, a.j.fold_chans, a.j.fold_patch,
                           static_cast<bf16_t*>(a.j.fold_out_bf16), bid, a.n_fold);
        return;
    }
    bid -= a.n_fold;
    if (bid < a.n_patch) {
        const bool bf = a.j.patch_dtype == SPV_BF16;
        if (!a.patch_vec4)
            patchify_body(a.j.patch_img, a.j.patch_out, a.j.patch_batch, a.j.patch_chans, a.j.patch_height, a.j.patch_width, a.j.patch_size,
                          a.j.patch_ld, 2, bf, bid, a.n_patch);
        else if (bf)
            patchify_vec4_body<bf16_t>(a.j.patch_img, static_cast<bf16_t*>(a.j.patch_out), a.j.patch_batch, a.j.patch_chans, a.j.patch_height,
                                       a.j.patch_width, a.j.patch_size, a.j.patch_ld, 1, bid, a.n_patch);
        else
            patchify_vec4_body<float>(a.j.patch_img, static_cast<float*>(a.j.patch_out), a.j.patch_batch, a.j.patch_chans, a.j.patch_height,
                                      a.j.patch_width, a.j.patch_size, a.j.patch_ld, 1, bid, a.n_patch);
        return;
    }
    bid -= a.n_patch;
    if (bid < a.n_pos) posbias_body(a.j.pos_pos, a.j.pos_bias, a.j.pos_cls, a.j.pos_out, a.j.pos_patches, a.j.pos_embed, bid, a.n_pos);
}
}
extern "C" int spv_set_seed_device_ptr(const void* seed_word) {
    const unsigned long long* p = static_cast<const unsigned long long*>(seed_word);
    SPV_CHECK(spv_seed_ptr_set_rowops(p) == 0 && spv_seed_ptr_set_patch(p) == 0 && spv_seed_ptr_set_attn(p) == 0 && spv_seed_ptr_set_gemm(p) == 0,
              "spv_set_seed_device_ptr: hipMemcpyToSymbol failed");
    return 0;
}
extern "C" int spv_seed_advance(void* seed_word, void* stream) {
    SPV_CHECK(seed_word != nullptr, "spv_seed_advance: null pointer");
    hipLaunchKernelGGL(seed_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), static_cast<unsigned long long*>(seed_word));
    SPV_LAUNCH_CHECK("spv_seed_advance");
    return 0;
}

extern "C" int spv_step_prologue(const spv_prologue_jobs* jobs, void* stream) {
    SPV_CHECK(jobs != nullptr, "spv_step_prologue: null jobs");
    PrologueArgs a;
    a.j = *jobs;
    const spv_prologue_jobs& j = a.j;
    a.n_seed = j.seed_word != nullptr ? 1 : 0;
    // shadows: the arrays of spv_weight_shadows_multi, one workgroup per tile
    SPV_CHECK(j.ntiles >= 0, "spv_step_prologue: ntiles = %d", j.ntiles);
    a.n_shadow = (j.shadow_table != nullptr && j.ntiles > 0) ? j.ntiles : 0;
    if (a.n_shadow) {
        SPV_CHECK(j.tile_tensor && j.tile_x && j.tile_y, "spv_step_prologue: null tile lists");
        SPV_CHECK(j.shadow_dtype == SPV_BF16 || j.shadow_dtype == SPV_F32, "spv_step_prologue: bad shadow dtype %d", j.shadow_dtype);
    }
    // spectral fold: spv_spectral_fold[_bf16]'s grid
    a.n_fold = 0;
    if (j.fold_w != nullptr && j.fold_embed > 0) {
        SPV_CHECK(j.fold_fh && j.fold_fw && j.fold_out && j.fold_chans > 0 && j.fold_patch > 0, "spv_step_prologue: bad spectral-fold arguments");
        a.n_fold = patch_ew_blocks((int64_t)j.fold_embed * j.fold_chans * j.fold_patch * j.fold_patch);
    }
    // patch rows in token layout (spv_patchify, transposed = 2): its shape checks, its choice of kernel, its grid
    a.n_patch = a.patch_vec4 = 0;
    if (j.patch_img != nullptr && j.patch_batch > 0) {
        SPV_CHECK(j.patch_out && j.patch_chans > 0 && j.patch_size > 0 && j.patch_height >= j.patch_size && j.patch_width >= j.patch_size,
                  "spv_step_prologue: bad patch shape");
        SPV_CHECK(j.patch_dtype == SPV_F32 || j.patch_dtype == SPV_BF16, "spv_step_prologue: bad patch dtype");
        const int Np = (j.patch_height / j.patch_size) * (j.patch_width / j.patch_size), K = j.patch_chans * j.patch_size * j.patch_size;
        SPV_CHECK(j.patch_ld >= K, "spv_step_prologue: patch ld=%d too small", j.patch_ld);
        if (j.patch_size % 4 == 0 && j.patch_width % 4 == 0 && j.patch_ld % 4 == 0 && ((uintptr_t)j.patch_img & 15) == 0 &&
            ((uintptr_t)j.patch_out & 15) == 0) {
            a.patch_vec4 = 1;
            a.n_patch = patch_ew_blocks((int64_t)j.patch_batch * (Np + 1) * (j.patch_ld / 4));
        } else {
            a.n_patch = patch_ew_blocks((int64_t)j.patch_batch * (Np + 1) * j.patch_ld);
        }
    }
    // position + bias rows (spv_embed_posbias)
    a.n_pos = 0;
    if (j.pos_pos != nullptr && j.pos_patches > 0) {
        SPV_CHECK(j.pos_bias && j.pos_out && j.pos_embed > 0, "spv_step_prologue: bad position-row arguments");
        a.n_pos = patch_ew_blocks((int64_t)(j.pos_patches + 1) * j.pos_embed);
    }
    const int64_t total = (int64_t)a.n_seed + a.n_shadow + a.n_fold + a.n_patch + a.n_pos;
    if (total == 0) return 0;
    SPV_CHECK(total < (1ll << 31), "spv_step_prologue: too many workgroups");
    hipLaunchKernelGGL(step_prologue_kernel, dim3((unsigned)total), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    SPV_LAUNCH_CHECK("spv_step_prologue");
    return 0;
}
