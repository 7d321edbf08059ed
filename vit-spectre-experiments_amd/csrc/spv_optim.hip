// spv_optim.hip -- on-device step control of the optimizer (include/spv.h: spv_step_ctl): the gradient's sum of squares (or, under
// gradient accumulation, the accumulator's, formed while the gradient is added to it), the one-workgroup kernel that turns it and the
// step counts into this step's learning rate / clip coefficient / apply flag, and the AdamW launch that reads them.  Nothing here is decided on the host, so a captured training step follows the schedule and skips a
// non-finite gradient on every replay.  At the end of the file: the launches of the two other update rules, torch.optim.Adam and
// torch.optim.SGD (spv_optim_rules.h), which read the same control block.
#include "spv_common.h"
#include "spv_adamw_core.h"
#include "spv_optim_rules.h"   // torch.optim.Adam and torch.optim.SGD on the same walk and the same control block (end of this file)

#include <math.h>

static_assert(sizeof(spv_step_ctl) == 64, "spv_step_ctl is a fixed 64-byte layout (spectre_vit/optim.py packs it by hand)");

namespace {
// ---------------------------------------------------------------------------------------------------------
// Sum of squares of one 2048-element gradient chunk, in fp64: the chunk walk of adamw_chunk (two float4 per thread where the
// gradient's base is 16-byte aligned, scalar otherwise and in the short last chunk of a tensor).  Fixed order: eight squares per
// thread, a butterfly over the wave, the four wave sums added by one thread.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                         const int* __restrict__ chunk_off, const int* __restrict__ sizes,
                                                         double* __restrict__ partials) {
    __shared__ double wave_part[4];
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const float* __restrict__ g = tab[t].g;
    const int n = sizes[t];
    const int base = off + threadIdx.x * 4;
    double s = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = base + h * 1024;
        if (i + 3 < n && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            const float4 q = *reinterpret_cast<const float4*>(g + i);
            s += (double)q.x * (double)q.x;
            s += (double)q.y * (double)q.y;
            s += (double)q.z * (double)q.z;
            s += (double)q.w * (double)q.w;
        } else {
            for (int u = 0; u < 4; ++u) {
                const int j = i + u;
                if (j >= n) break;
                const double x = (double)g[j];
                s += x * x;
            }
        }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

// ---------------------------------------------------------------------------------------------------------
// Gradient accumulation: the same chunk walk with the accumulator taken along.  ctl->micro == 0 opens a window: acc = g, an
// assignment that does not read the old accumulator (whatever a dropped window left there, a NaN included, is gone).  Otherwise
// acc = acc + g, one fp32 add per element.  The chunk's sum of squares is that of the NEW accumulator, in grad_sumsq_kernel's order
// (with micro == 0 its very bits).  An accumulator slot is 16-byte aligned and padded to four elements, so wherever g takes the
// float4 branch (i + 3 < n) the accumulator's float4 at the same index is aligned and inside its slot; an unaligned g takes the
// scalar branch for both.
__global__ __launch_bounds__(256) void grad_accumulate_kernel(const AdamTensor* __restrict__ tab, float* const* __restrict__ acc_tab,
                                                              const int* __restrict__ chunk_tensor, const int* __restrict__ chunk_off,
                                                              const int* __restrict__ sizes, const spv_step_ctl* __restrict__ ctl,
                                                              double* __restrict__ partials) {
    __shared__ double wave_part[4];
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const float* __restrict__ g = tab[t].g;
    float* __restrict__ acc = acc_tab[t];
    const int n = sizes[t];
    const bool open = ctl->micro == 0;
    const int base = off + threadIdx.x * 4;
    double s = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = base + h * 1024;
        if (i + 3 < n && (reinterpret_cast<uintptr_t>(g) & 15) == 0) {
            float4 q = *reinterpret_cast<const float4*>(g + i);
            if (!open) {
                const float4 a = *reinterpret_cast<const float4*>(acc + i);
                q.x = a.x + q.x;
                q.y = a.y + q.y;
                q.z = a.z + q.z;
                q.w = a.w + q.w;
            }
            *reinterpret_cast<float4*>(acc + i) = q;
            s += (double)q.x * (double)q.x;
            s += (double)q.y * (double)q.y;
            s += (double)q.z * (double)q.z;
            s += (double)q.w * (double)q.w;
        } else {
            for (int u = 0; u < 4; ++u) {
                const int j = i + u;
                if (j >= n) break;
                float v = g[j];
                if (!open) v = acc[j] + v;
                acc[j] = v;
                const double x = (double)v;
                s += x * x;
            }
        }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
}

// ---------------------------------------------------------------------------------------------------------
// One workgroup: partials -> ctl.  Thread i adds partials i, i + 256, ... in that order, a fixed tree joins the 256 sums; the same
// launch gives the same bits on every replay and on every rank of a data-parallel job (each holds the same averaged gradient).
// ACCUM: a window of accum_k micro-steps (include/spv.h: spv_step_control_accum).  Inside the window only apply and micro are
// written; at its boundary the block is filled as without accumulation, from the norm of the mean gradient, and the clip
// coefficient carries the 1 / accum_k that turns the summed gradient into the mean.  Both divisions are exact for accum_k = 1.
template <bool ACCUM>
__global__ __launch_bounds__(256) void step_control_kernel(const double* __restrict__ partials, int npartials, float* const* __restrict__ step_ptrs,
                                                           int nsteps, spv_step_ctl* __restrict__ ctl, int flags, int warmup_steps,
                                                           int total_steps, double eta_min, float max_norm, int accum_k) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < npartials; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if constexpr (ACCUM) {
        const int micro = ctl->micro;
        if (micro < accum_k - 1) {   // inside the window: the optimizer launch writes nothing, the last boundary's values stay
            ctl->apply = 0;
            ctl->micro = micro + 1;
            return;
        }
        ctl->micro = 0;
    }
    const double sumsq = red[0];
    const float norm = ACCUM ? (float)(sqrt(sumsq) / (double)accum_k) : (float)sqrt(sumsq);
    const int t = ctl->sched_step;
    double a = 1.0, b = 0.0;
    if (flags & SPV_CTL_SCHEDULE) {
        if (t < warmup_steps) {
            a = (double)(t + 1) / (double)(warmup_steps + 1);
        } else {
            const int span = total_steps - warmup_steps;
            const int k = min(t - warmup_steps, span);
            a = k >= span ? 0.0 : 0.5 * (1.0 + cos(M_PI * (double)k / (double)span));   // past T: exactly eta_min
            b = eta_min * (1.0 - a);
        }
    }
    float coef = 1.0f;
    if (flags & SPV_CTL_CLIP) {
        const float c = max_norm / (norm + 1e-6f);
        coef = c < 1.0f ? c : (c != c ? c : 1.0f);   // clamp(max=1) that keeps a NaN, as torch's
    }
    if constexpr (ACCUM) coef = (float)((double)coef / (double)accum_k);
    const int apply = ((flags & SPV_CTL_SKIP_NONFINITE) && !isfinite(sumsq)) ? 0 : 1;
    ctl->a = a;
    ctl->b = b;
    ctl->clip_coef = coef;
    ctl->apply = apply;
    ctl->grad_norm = norm;
    ctl->sched_step = t + 1;
    if (apply) {
        for (int k = 0; k < nsteps; ++k) *step_ptrs[k] += 1.0f;
    } else {
        ctl->skipped += 1;
    }
}

__global__ __launch_bounds__(256) void adamw_multi_ctl_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                              const int* __restrict__ chunk_off, const int* __restrict__ sizes, double base_lr,
                                                              float beta1, float beta2, float omb1, float omb2, float eps, float wd,
                                                              const float* __restrict__ step_dev, const spv_step_ctl* __restrict__ ctl) {
    if (ctl->apply == 0) return;   // a dropped step writes nothing
    // product and sum rounded separately (no fused multiply-add): the host reproduces the rate from a, b bit for bit
    const float lr = (float)__dadd_rn(__dmul_rn(ctl->a, base_lr), ctl->b);
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const AdamTensor a = tab[t];
    const int n = sizes[t];
    adamw_chunk<true>(a, n, off, lr, beta1, beta2, omb1, omb2, eps, wd, 0.0f, 0.0f, step_dev, ctl->clip_coef);
}

// The same launch with the weights' moving average (spv_adamw_core.h: EMA); a dropped step leaves the average where it is.
__global__ __launch_bounds__(256) void adamw_multi_ctl_ema_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                                  const int* __restrict__ chunk_off, const int* __restrict__ sizes, double base_lr,
                                                                  float beta1, float beta2, float omb1, float omb2, float eps, float wd,
                                                                  const float* __restrict__ step_dev, const spv_step_ctl* __restrict__ ctl,
                                                                  float* const* __restrict__ ema_tab, float ema_w, int ema_warmup) {
    if (ctl->apply == 0) return;
    const float lr = (float)__dadd_rn(__dmul_rn(ctl->a, base_lr), ctl->b);
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const AdamTensor a = tab[t];
    const int n = sizes[t];
    adamw_chunk<true, true>(a, n, off, lr, beta1, beta2, omb1, omb2, eps, wd, 0.0f, 0.0f, step_dev, ctl->clip_coef, ema_tab[t], ema_w,
                            ema_warmup, 0.0f);
}

// ---------------------------------------------------------------------------------------------------------
// The two other update rules of the reference's script on the same walk (spv_optim_rules.h): torch.optim.Adam and torch.optim.SGD,
// each as a launch that takes the rate by value and as one that reads rate, gradient scale and the apply flag from the control
// block, with and without the weights' moving average (EMA: ema_tab is read only then).
template <bool EMA>
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                         const int* __restrict__ chunk_off, const int* __restrict__ sizes, float lr,
                                                         float beta1, float beta2, float omb1, float omb2, float eps, float wd, float bc1,
                                                         float bc2, const float* __restrict__ step_dev, float* const* __restrict__ ema_tab,
                                                         float ema_w, int ema_warmup, float ema_step) {
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const AdamTensor a = tab[t];
    const int n = sizes[t];
    adam_chunk<false, EMA>(a, n, off, lr, beta1, beta2, omb1, omb2, eps, wd, bc1, bc2, step_dev, 1.0f, EMA ? ema_tab[t] : nullptr, ema_w,
                           ema_warmup, ema_step);
}

template <bool EMA>
__global__ __launch_bounds__(256) void adam_multi_ctl_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                             const int* __restrict__ chunk_off, const int* __restrict__ sizes, double base_lr,
                                                             float beta1, float beta2, float omb1, float omb2, float eps, float wd,
                                                             const float* __restrict__ step_dev, const spv_step_ctl* __restrict__ ctl,
                                                             float* const* __restrict__ ema_tab, float ema_w, int ema_warmup) {
    if (ctl->apply == 0) return;   // a dropped step writes nothing
    const float lr = (float)__dadd_rn(__dmul_rn(ctl->a, base_lr), ctl->b);
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const AdamTensor a = tab[t];
    const int n = sizes[t];
    adam_chunk<true, EMA>(a, n, off, lr, beta1, beta2, omb1, omb2, eps, wd, 0.0f, 0.0f, step_dev, ctl->clip_coef,
                          EMA ? ema_tab[t] : nullptr, ema_w, ema_warmup, 0.0f);
}

// SGD: s = this step's count of the group (already advanced), *step_dev or -- step_dev == NULL -- `step` by value.  s == 1 is the
// first applied step, where the momentum buffer is assigned and not read.
template <bool EMA>
__global__ __launch_bounds__(256) void sgd_multi_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                        const int* __restrict__ chunk_off, const int* __restrict__ sizes, float lr,
                                                        float momentum, float omd, float wd, int nesterov, float step,
                                                        const float* __restrict__ step_dev, float* const* __restrict__ ema_tab, float ema_w,
                                                        int ema_warmup) {
    const float s = step_dev != nullptr ? *step_dev : step;
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const AdamTensor a = tab[t];
    const int n = sizes[t];
    const SgdRule r = {lr, momentum, omd, wd, nesterov != 0, s == 1.0f};
    sgd_chunk<false, EMA>(a, n, off, r, s, 1.0f, EMA ? ema_tab[t] : nullptr, ema_w, ema_warmup);
}

template <bool EMA>
__global__ __launch_bounds__(256) void sgd_multi_ctl_kernel(const AdamTensor* __restrict__ tab, const int* __restrict__ chunk_tensor,
                                                            const int* __restrict__ chunk_off, const int* __restrict__ sizes, double base_lr,
                                                            float momentum, float omd, float wd, int nesterov,
                                                            const float* __restrict__ step_dev, const spv_step_ctl* __restrict__ ctl,
                                                            float* const* __restrict__ ema_tab, float ema_w, int ema_warmup) {
    if (ctl->apply == 0) return;   // a dropped step writes nothing: no parameter, no buffer, no average
    const float lr = (float)__dadd_rn(__dmul_rn(ctl->a, base_lr), ctl->b);
    const float s = *step_dev;
    const int t = chunk_tensor[blockIdx.x];
    const int off = chunk_off[blockIdx.x];
    const AdamTensor a = tab[t];
    const int n = sizes[t];
    const SgdRule r = {lr, momentum, omd, wd, nesterov != 0, s == 1.0f};
    sgd_chunk<true, EMA>(a, n, off, r, s, ctl->clip_coef, EMA ? ema_tab[t] : nullptr, ema_w, ema_warmup);
}
}  // namespace

extern "C" int spv_grad_sumsq(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                              double* partials, void* stream) {
    SPV_CHECK(nchunks >= 0, "spv_grad_sumsq: nchunks = %d", nchunks);
    SPV_CHECK(table && chunk_tensor && chunk_off && sizes, "spv_grad_sumsq: null table");
    SPV_CHECK(partials, "spv_grad_sumsq: null partials");
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, partials);
    SPV_LAUNCH_CHECK("spv_grad_sumsq");
    return 0;
}

extern "C" int spv_step_control(const double* partials, int npartials, float* const* step_ptrs, int nsteps, spv_step_ctl* ctl, int flags,
                                int warmup_steps, int total_steps, double eta_min, float max_norm, void* stream) {
    SPV_CHECK(npartials >= 0 && nsteps >= 0, "spv_step_control: npartials = %d, nsteps = %d", npartials, nsteps);
    SPV_CHECK(ctl, "spv_step_control: null control block");
    SPV_CHECK((partials || npartials == 0) && (step_ptrs || nsteps == 0), "spv_step_control: null partials / step_ptrs");
    SPV_CHECK((flags & ~(SPV_CTL_SCHEDULE | SPV_CTL_CLIP | SPV_CTL_SKIP_NONFINITE)) == 0, "spv_step_control: unknown flags 0x%x", flags);
    if (flags & SPV_CTL_SCHEDULE) {
        SPV_CHECK(warmup_steps >= 0 && total_steps > warmup_steps, "spv_step_control: schedule needs 0 <= warmup_steps < total_steps (%d, %d)",
                  warmup_steps, total_steps);
        SPV_CHECK(eta_min >= 0.0, "spv_step_control: eta_min = %g must be >= 0", eta_min);   // (false for a NaN too)
    }
    if (flags & SPV_CTL_CLIP) SPV_CHECK(max_norm > 0.0f, "spv_step_control: max_norm = %g must be > 0", (double)max_norm);
    hipLaunchKernelGGL(step_control_kernel<false>, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), partials, npartials, step_ptrs,
                       nsteps, ctl, flags, warmup_steps, total_steps, eta_min, max_norm, 1);
    SPV_LAUNCH_CHECK("spv_step_control");
    return 0;
}

extern "C" int spv_grad_accumulate(const void* table, float* const* acc_table, const int* chunk_tensor, const int* chunk_off,
                                   const int* sizes, int nchunks, const spv_step_ctl* ctl, double* partials, void* stream) {
    SPV_CHECK(nchunks >= 0, "spv_grad_accumulate: nchunks = %d", nchunks);
    SPV_CHECK(table && chunk_tensor && chunk_off && sizes, "spv_grad_accumulate: null table");
    SPV_CHECK(acc_table, "spv_grad_accumulate: null acc_table");
    SPV_CHECK(ctl, "spv_grad_accumulate: null control block");
    SPV_CHECK(partials, "spv_grad_accumulate: null partials");
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), acc_table, chunk_tensor, chunk_off, sizes, ctl, partials);
    SPV_LAUNCH_CHECK("spv_grad_accumulate");
    return 0;
}

extern "C" int spv_step_control_accum(const double* partials, int npartials, float* const* step_ptrs, int nsteps, spv_step_ctl* ctl,
                                      int flags, int warmup_steps, int total_steps, double eta_min, float max_norm, int accumulate_steps,
                                      void* stream) {
    SPV_CHECK(npartials >= 0 && nsteps >= 0, "spv_step_control_accum: npartials = %d, nsteps = %d", npartials, nsteps);
    SPV_CHECK(ctl, "spv_step_control_accum: null control block");
    SPV_CHECK((partials || npartials == 0) && (step_ptrs || nsteps == 0), "spv_step_control_accum: null partials / step_ptrs");
    SPV_CHECK((flags & ~(SPV_CTL_SCHEDULE | SPV_CTL_CLIP | SPV_CTL_SKIP_NONFINITE)) == 0, "spv_step_control_accum: unknown flags 0x%x", flags);
    SPV_CHECK(accumulate_steps >= 1, "spv_step_control_accum: accumulate_steps = %d must be >= 1", accumulate_steps);
    if (flags & SPV_CTL_SCHEDULE) {
        SPV_CHECK(warmup_steps >= 0 && total_steps > warmup_steps,
                  "spv_step_control_accum: schedule needs 0 <= warmup_steps < total_steps (%d, %d)", warmup_steps, total_steps);
        SPV_CHECK(eta_min >= 0.0, "spv_step_control_accum: eta_min = %g must be >= 0", eta_min);
    }
    if (flags & SPV_CTL_CLIP) SPV_CHECK(max_norm > 0.0f, "spv_step_control_accum: max_norm = %g must be > 0", (double)max_norm);
    hipLaunchKernelGGL(step_control_kernel<true>, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), partials, npartials, step_ptrs,
                       nsteps, ctl, flags, warmup_steps, total_steps, eta_min, max_norm, accumulate_steps);
    SPV_LAUNCH_CHECK("spv_step_control_accum");
    return 0;
}

extern "C" int spv_adamw_multi_ctl(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                                   double base_lr, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                                   float weight_decay, const float* step_dev, const spv_step_ctl* ctl, void* stream) {
    SPV_CHECK(nchunks >= 0, "spv_adamw_multi_ctl: nchunks = %d", nchunks);
    SPV_CHECK(table && chunk_tensor && chunk_off && sizes, "spv_adamw_multi_ctl: null table");
    SPV_CHECK(step_dev && ctl, "spv_adamw_multi_ctl: null step count / control block");
    SPV_CHECK(base_lr >= 0.0, "spv_adamw_multi_ctl: base_lr = %g must be >= 0", base_lr);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(adamw_multi_ctl_kernel, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, base_lr, beta1, beta2, one_minus_beta1,
                       one_minus_beta2, eps, weight_decay, step_dev, ctl);
    SPV_LAUNCH_CHECK("spv_adamw_multi_ctl");
    return 0;
}

extern "C" int spv_adamw_multi_ctl_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                                       double base_lr, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                                       float weight_decay, const float* step_dev, const spv_step_ctl* ctl, float* const* ema_table,
                                       float ema_weight, int ema_warmup, void* stream) {
    SPV_CHECK(nchunks >= 0, "spv_adamw_multi_ctl_ema: nchunks = %d", nchunks);
    SPV_CHECK(table && chunk_tensor && chunk_off && sizes, "spv_adamw_multi_ctl_ema: null table");
    SPV_CHECK(step_dev && ctl, "spv_adamw_multi_ctl_ema: null step count / control block");
    SPV_CHECK(ema_table, "spv_adamw_multi_ctl_ema: null ema_table (use spv_adamw_multi_ctl for a group that is not averaged)");
    SPV_CHECK(base_lr >= 0.0, "spv_adamw_multi_ctl_ema: base_lr = %g must be >= 0", base_lr);
    SPV_CHECK(ema_weight > 0.0f && ema_weight <= 1.0f, "spv_adamw_multi_ctl_ema: ema_weight = %g must be in (0, 1]", (double)ema_weight);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(adamw_multi_ctl_ema_kernel, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, base_lr, beta1, beta2, one_minus_beta1,
                       one_minus_beta2, eps, weight_decay, step_dev, ctl, ema_table, ema_weight, ema_warmup);
    SPV_LAUNCH_CHECK("spv_adamw_multi_ctl_ema");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// torch.optim.Adam and torch.optim.SGD: the checks every form of a rule shares, then the eight entry points.
namespace {
int adam_args_ok(const char* who, const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                 float beta1, float beta2, float eps, float wd) {
    SPV_CHECK(nchunks >= 0, "%s: nchunks = %d", who, nchunks);
    SPV_CHECK(table && chunk_tensor && chunk_off && sizes, "%s: null table", who);
    SPV_CHECK(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f, "%s: betas (%g, %g) must be in [0, 1)", who, (double)beta1,
              (double)beta2);
    SPV_CHECK(eps >= 0.0f && wd >= 0.0f, "%s: eps = %g and weight_decay = %g must be >= 0", who, (double)eps, (double)wd);
    return 0;
}

int sgd_args_ok(const char* who, const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                float momentum, float omd, float wd, int nesterov) {
    SPV_CHECK(nchunks >= 0, "%s: nchunks = %d", who, nchunks);
    SPV_CHECK(table && chunk_tensor && chunk_off && sizes, "%s: null table", who);
    SPV_CHECK(momentum >= 0.0f && momentum < 1.0f, "%s: momentum = %g must be in [0, 1)", who, (double)momentum);
    SPV_CHECK(omd > 0.0f && omd <= 1.0f, "%s: one_minus_dampening = %g must be in (0, 1] (dampening in [0, 1))", who, (double)omd);
    SPV_CHECK(wd >= 0.0f, "%s: weight_decay = %g must be >= 0", who, (double)wd);
    SPV_CHECK(!nesterov || (momentum > 0.0f && omd == 1.0f), "%s: nesterov needs momentum > 0 and dampening == 0", who);
    return 0;
}

int ema_args_ok(const char* who, float* const* ema_table, float ema_weight) {
    SPV_CHECK(ema_table, "%s: null ema_table (use the form without _ema for a group that is not averaged)", who);
    SPV_CHECK(ema_weight > 0.0f && ema_weight <= 1.0f, "%s: ema_weight = %g must be in (0, 1]", who, (double)ema_weight);
    return 0;
}
}  // namespace

#define SPV_RULE_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

extern "C" int spv_adam_multi(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                              float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                              float bias_correction1, float bias_correction2, const float* step_dev, void* stream) {
    SPV_RULE_TRY(adam_args_ok("spv_adam_multi", table, chunk_tensor, chunk_off, sizes, nchunks, beta1, beta2, eps, weight_decay));
    SPV_CHECK(lr >= 0.0f, "spv_adam_multi: lr = %g must be >= 0", (double)lr);
    SPV_CHECK(step_dev != nullptr || (bias_correction1 > 0.0f && bias_correction2 > 0.0f), "spv_adam_multi: bias corrections must be > 0");
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(adam_multi_kernel<false>, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, lr, beta1, beta2, one_minus_beta1,
                       one_minus_beta2, eps, weight_decay, bias_correction1, bias_correction2, step_dev,
                       static_cast<float* const*>(nullptr), 0.0f, 0, 0.0f);
    SPV_LAUNCH_CHECK("spv_adam_multi");
    return 0;
}

extern "C" int spv_adam_multi_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                                  float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, float weight_decay,
                                  float bias_correction1, float bias_correction2, const float* step_dev, float* const* ema_table,
                                  float ema_weight, int ema_warmup, float ema_step, void* stream) {
    SPV_RULE_TRY(adam_args_ok("spv_adam_multi_ema", table, chunk_tensor, chunk_off, sizes, nchunks, beta1, beta2, eps, weight_decay));
    SPV_RULE_TRY(ema_args_ok("spv_adam_multi_ema", ema_table, ema_weight));
    SPV_CHECK(lr >= 0.0f, "spv_adam_multi_ema: lr = %g must be >= 0", (double)lr);
    SPV_CHECK(step_dev != nullptr || (bias_correction1 > 0.0f && bias_correction2 > 0.0f), "spv_adam_multi_ema: bias corrections must be > 0");
    SPV_CHECK(!ema_warmup || step_dev != nullptr || ema_step >= 1.0f, "spv_adam_multi_ema: ema_step = %g must be >= 1 (the step count of this step)",
              (double)ema_step);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(adam_multi_kernel<true>, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, lr, beta1, beta2, one_minus_beta1,
                       one_minus_beta2, eps, weight_decay, bias_correction1, bias_correction2, step_dev, ema_table, ema_weight, ema_warmup,
                       ema_step);
    SPV_LAUNCH_CHECK("spv_adam_multi_ema");
    return 0;
}

extern "C" int spv_adam_multi_ctl(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                                  double base_lr, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                                  float weight_decay, const float* step_dev, const spv_step_ctl* ctl, void* stream) {
    SPV_RULE_TRY(adam_args_ok("spv_adam_multi_ctl", table, chunk_tensor, chunk_off, sizes, nchunks, beta1, beta2, eps, weight_decay));
    SPV_CHECK(step_dev && ctl, "spv_adam_multi_ctl: null step count / control block");
    SPV_CHECK(base_lr >= 0.0, "spv_adam_multi_ctl: base_lr = %g must be >= 0", base_lr);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(adam_multi_ctl_kernel<false>, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, base_lr, beta1, beta2, one_minus_beta1,
                       one_minus_beta2, eps, weight_decay, step_dev, ctl, static_cast<float* const*>(nullptr), 0.0f, 0);
    SPV_LAUNCH_CHECK("spv_adam_multi_ctl");
    return 0;
}

extern "C" int spv_adam_multi_ctl_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                                      double base_lr, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                                      float weight_decay, const float* step_dev, const spv_step_ctl* ctl, float* const* ema_table,
                                      float ema_weight, int ema_warmup, void* stream) {
    SPV_RULE_TRY(adam_args_ok("spv_adam_multi_ctl_ema", table, chunk_tensor, chunk_off, sizes, nchunks, beta1, beta2, eps, weight_decay));
    SPV_RULE_TRY(ema_args_ok("spv_adam_multi_ctl_ema", ema_table, ema_weight));
    SPV_CHECK(step_dev && ctl, "spv_adam_multi_ctl_ema: null step count / control block");
    SPV_CHECK(base_lr >= 0.0, "spv_adam_multi_ctl_ema: base_lr = %g must be >= 0", base_lr);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(adam_multi_ctl_kernel<true>, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, base_lr, beta1, beta2, one_minus_beta1,
                       one_minus_beta2, eps, weight_decay, step_dev, ctl, ema_table, ema_weight, ema_warmup);
    SPV_LAUNCH_CHECK("spv_adam_multi_ctl_ema");
    return 0;
}

extern "C" int spv_sgd_multi(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                             float momentum, float one_minus_dampening, float weight_decay, int nesterov, float step, const float* step_dev,
                             void* stream) {
    SPV_RULE_TRY(sgd_args_ok("spv_sgd_multi", table, chunk_tensor, chunk_off, sizes, nchunks, momentum, one_minus_dampening, weight_decay,
                             nesterov));
    SPV_CHECK(lr >= 0.0f, "spv_sgd_multi: lr = %g must be >= 0", (double)lr);
    SPV_CHECK(step_dev != nullptr || step >= 1.0f, "spv_sgd_multi: null step count and step = %g (this step's count, >= 1)", (double)step);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(sgd_multi_kernel<false>, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, lr, momentum, one_minus_dampening, weight_decay,
                       nesterov, step, step_dev, static_cast<float* const*>(nullptr), 0.0f, 0);
    SPV_LAUNCH_CHECK("spv_sgd_multi");
    return 0;
}

extern "C" int spv_sgd_multi_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks, float lr,
                                 float momentum, float one_minus_dampening, float weight_decay, int nesterov, float step,
                                 const float* step_dev, float* const* ema_table, float ema_weight, int ema_warmup, void* stream) {
    SPV_RULE_TRY(sgd_args_ok("spv_sgd_multi_ema", table, chunk_tensor, chunk_off, sizes, nchunks, momentum, one_minus_dampening,
                             weight_decay, nesterov));
    SPV_RULE_TRY(ema_args_ok("spv_sgd_multi_ema", ema_table, ema_weight));
    SPV_CHECK(lr >= 0.0f, "spv_sgd_multi_ema: lr = %g must be >= 0", (double)lr);
    SPV_CHECK(step_dev != nullptr || step >= 1.0f, "spv_sgd_multi_ema: null step count and step = %g (this step's count, >= 1)", (double)step);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(sgd_multi_kernel<true>, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, lr, momentum, one_minus_dampening, weight_decay,
                       nesterov, step, step_dev, ema_table, ema_weight, ema_warmup);
    SPV_LAUNCH_CHECK("spv_sgd_multi_ema");
    return 0;
}

extern "C" int spv_sgd_multi_ctl(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                                 double base_lr, float momentum, float one_minus_dampening, float weight_decay, int nesterov,
                                 const float* step_dev, const spv_step_ctl* ctl, void* stream) {
    SPV_RULE_TRY(sgd_args_ok("spv_sgd_multi_ctl", table, chunk_tensor, chunk_off, sizes, nchunks, momentum, one_minus_dampening,
                             weight_decay, nesterov));
    SPV_CHECK(step_dev && ctl, "spv_sgd_multi_ctl: null step count / control block");
    SPV_CHECK(base_lr >= 0.0, "spv_sgd_multi_ctl: base_lr = %g must be >= 0", base_lr);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(sgd_multi_ctl_kernel<false>, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, base_lr, momentum, one_minus_dampening,
                       weight_decay, nesterov, step_dev, ctl, static_cast<float* const*>(nullptr), 0.0f, 0);
    SPV_LAUNCH_CHECK("spv_sgd_multi_ctl");
    return 0;
}

extern "C" int spv_sgd_multi_ctl_ema(const void* table, const int* chunk_tensor, const int* chunk_off, const int* sizes, int nchunks,
                                     double base_lr, float momentum, float one_minus_dampening, float weight_decay, int nesterov,
                                     const float* step_dev, const spv_step_ctl* ctl, float* const* ema_table, float ema_weight,
                                     int ema_warmup, void* stream) {
    SPV_RULE_TRY(sgd_args_ok("spv_sgd_multi_ctl_ema", table, chunk_tensor, chunk_off, sizes, nchunks, momentum, one_minus_dampening,
                             weight_decay, nesterov));
    SPV_RULE_TRY(ema_args_ok("spv_sgd_multi_ctl_ema", ema_table, ema_weight));
    SPV_CHECK(step_dev && ctl, "spv_sgd_multi_ctl_ema: null step count / control block");
    SPV_CHECK(base_lr >= 0.0, "spv_sgd_multi_ctl_ema: base_lr = %g must be >= 0", base_lr);
    if (nchunks == 0) return 0;
    hipLaunchKernelGGL(sgd_multi_ctl_kernel<true>, dim3(nchunks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const AdamTensor*>(table), chunk_tensor, chunk_off, sizes, base_lr, momentum, one_minus_dampening,
                       weight_decay, nesterov, step_dev, ctl, ema_table, ema_weight, ema_warmup);
    SPV_LAUNCH_CHECK("spv_sgd_multi_ctl_ema");
    return 0;
}
