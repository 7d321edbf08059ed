// The AdamW update of one 2048-element chunk: ONE body for both optimizer launches -- adamw_multi_kernel (spv_misc.hip: the
// learning rate by value) and adamw_multi_ctl_kernel (spv_optim.hip: learning rate, gradient scale and the apply flag from the
// device-side step-control block).  Arithmetic = torch.optim.AdamW (decoupled weight decay, bias correction, amsgrad off,
// maximize off).
#pragma once
#include "spv_common.h"

struct AdamTensor { float* p; const float* g; float* m; float* v; };

constexpr int ADAM_CHUNK = 2048;  // elements per workgroup: 256 threads x 2 x float4 (spectre_vit/optim.py: _CHUNK)

// Workgroup `blockIdx.x` updates elements [off, off + 2048) of tensor `a` (n elements); vectorised when all four bases are 16-byte
// aligned, scalar otherwise and in a tensor's short tail.  step_dev != NULL (capturable mode): the bias corrections come from the
// device-side step count (already advanced for this step).  SCALED: the gradient is multiplied by gscale in registers (the clip
// coefficient; g itself is not rewritten) -- with gscale = 1.0f the update is bit for bit the unscaled one.
template <bool SCALED>
__device__ __forceinline__ void adamw_chunk(const AdamTensor a, int n, int off, float lr, float beta1, float beta2, float omb1, float omb2,
                                            float eps, float wd, float bc1, float bc2, const float* __restrict__ step_dev, float gscale) {
    // No implicit contraction in here: every fused multiply-add is spelled out (they are the forms the compiler had chosen for the
    // shipped kernel, which differ between the vector and the scalar walk), so that both instantiations round alike.
#pragma clang fp contract(off)
    if (step_dev != nullptr) {  // capturable mode: the step count lives on the device (already advanced for this step)
        const float s = *step_dev;
        bc1 = 1.0f - powf(beta1, s);
        bc2 = 1.0f - powf(beta2, s);
    }
    const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2), decay = fmaf(-lr, wd, 1.0f);
    const int base = off + threadIdx.x * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = base + h * 1024;
        if (i + 3 < n && ((reinterpret_cast<uintptr_t>(a.p) | reinterpret_cast<uintptr_t>(a.g) | reinterpret_cast<uintptr_t>(a.m) |
                           reinterpret_cast<uintptr_t>(a.v)) & 15) == 0) {
            float4 p = *reinterpret_cast<const float4*>(a.p + i), m = *reinterpret_cast<const float4*>(a.m + i);
            float4 v = *reinterpret_cast<const float4*>(a.v + i);
            const float4 g = *reinterpret_cast<const float4*>(a.g + i);
            float* pp = &p.x; float* mm = &m.x; float* vv = &v.x; const float* gg = &g.x;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float gu = SCALED ? gg[u] * gscale : gg[u];
                mm[u] = fmaf(beta1, mm[u], omb1 * gu);
                vv[u] = fmaf(omb2 * gu, gu, beta2 * vv[u]);
                pp[u] = fmaf(pp[u], decay, -(step_size * mm[u] / fmaf(sqrtf(vv[u]), inv_sqrt_bc2, eps)));
            }
            *reinterpret_cast<float4*>(a.p + i) = p;
            *reinterpret_cast<float4*>(a.m + i) = m;
            *reinterpret_cast<float4*>(a.v + i) = v;
        } else {
            for (int u = 0; u < 4; ++u) {
                const int j = i + u;
                if (j >= n) break;
                const float g = SCALED ? a.g[j] * gscale : a.g[j];
                const float m = fmaf(omb1, g, beta1 * a.m[j]);
                const float v = beta2 * a.v[j] + omb2 * g * g;
                a.m[j] = m;
                a.v[j] = v;
                a.p[j] = a.p[j] * decay - step_size * m / fmaf(sqrtf(v), inv_sqrt_bc2, eps);
            }
        }
    }
}
