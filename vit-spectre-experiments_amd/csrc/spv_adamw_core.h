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
//
// EMA: the exponential moving average e of the weights (include/spv.h: spv_adamw_multi_ema), updated from the registers that hold
// the new weight p':  e' = fmaf(w_t, p' - e, e), w_t = ema_w or -- ema_warmup -- max(ema_w, 9 / (10 + s)), s = the step count of this
// step (*step_dev, or ema_step by value).  e == NULL: this tensor is not averaged.  p, g, m and v are walked exactly as with
// EMA = false -- the vector and the scalar walk round m and p differently, so the walk must not depend on e or the average would
// perturb the training it follows; an e that is not 16-byte aligned is read and written element by element inside the vector walk.
// The e arithmetic is the same expression on every path.
//
// L2: torch.optim.Adam's rule (spv_optim_rules.h: adam_chunk) -- the decay joins the gradient, d = g + wd * p (product and sum rounded
// separately, skipped when wd == 0, as torch's grad.add(p, alpha=wd)), and the decoupled factor is 1.  Every other expression is the
// one AdamW uses, so with wd == 0 the two rules give the same bits on either walk.
template <bool SCALED, bool EMA = false, bool L2 = false>
__device__ __forceinline__ void adamw_chunk(const AdamTensor a, int n, int off, float lr, float beta1, float beta2, float omb1, float omb2,
                                            float eps, float wd, float bc1, float bc2, const float* __restrict__ step_dev, float gscale,
                                            float* __restrict__ e = nullptr, float ema_w = 0.0f, int ema_warmup = 0,
                                            float ema_step = 0.0f) {
    // No implicit contraction in here: every fused multiply-add is spelled out (they are the forms the compiler had chosen for the
    // shipped kernel, which differ between the vector and the scalar walk), so that both instantiations round alike.
#pragma clang fp contract(off)
    if (step_dev != nullptr) {  // capturable mode: the step count lives on the device (already advanced for this step)
        const float s = *step_dev;
        bc1 = 1.0f - powf(beta1, s);
        bc2 = 1.0f - powf(beta2, s);
    }
    const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2), decay = L2 ? 1.0f : fmaf(-lr, wd, 1.0f);
    const bool l2 = L2 && wd != 0.0f;
    float w_t = ema_w;
    if (EMA && ema_warmup) w_t = fmaxf(ema_w, 9.0f / (10.0f + (step_dev != nullptr ? *step_dev : ema_step)));
    const bool averaged = EMA && e != nullptr;
    const bool e_vec = (reinterpret_cast<uintptr_t>(e) & 15) == 0;
    const int base = off + threadIdx.x * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = base + h * 1024;
        if (i + 3 < n && ((reinterpret_cast<uintptr_t>(a.p) | reinterpret_cast<uintptr_t>(a.g) | reinterpret_cast<uintptr_t>(a.m) |
                           reinterpret_cast<uintptr_t>(a.v)) & 15) == 0) {
            float4 p = *reinterpret_cast<const float4*>(a.p + i), m = *reinterpret_cast<const float4*>(a.m + i);
            float4 v = *reinterpret_cast<const float4*>(a.v + i);
            const float4 g = *reinterpret_cast<const float4*>(a.g + i);
            float4 ev = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (averaged) {
                if (e_vec) ev = *reinterpret_cast<const float4*>(e + i);
                else ev = make_float4(e[i], e[i + 1], e[i + 2], e[i + 3]);
            }
            float* pp = &p.x; float* mm = &m.x; float* vv = &v.x; const float* gg = &g.x; float* ee = &ev.x;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float gu = SCALED ? gg[u] * gscale : gg[u];
                if (L2 && l2) {
                    const float t = wd * pp[u];
                    gu = gu + t;
                }
                mm[u] = fmaf(beta1, mm[u], omb1 * gu);
                vv[u] = fmaf(omb2 * gu, gu, beta2 * vv[u]);
                pp[u] = fmaf(pp[u], decay, -(step_size * mm[u] / fmaf(sqrtf(vv[u]), inv_sqrt_bc2, eps)));
                if (EMA) ee[u] = fmaf(w_t, pp[u] - ee[u], ee[u]);
            }
            *reinterpret_cast<float4*>(a.p + i) = p;
            *reinterpret_cast<float4*>(a.m + i) = m;
            *reinterpret_cast<float4*>(a.v + i) = v;
            if (averaged) {
                if (e_vec) {
                    *reinterpret_cast<float4*>(e + i) = ev;
                } else {
                    e[i] = ev.x; e[i + 1] = ev.y; e[i + 2] = ev.z; e[i + 3] = ev.w;
                }
            }
        } else {
            for (int u = 0; u < 4; ++u) {
                const int j = i + u;
                if (j >= n) break;
                float g = SCALED ? a.g[j] * gscale : a.g[j];
                if (L2 && l2) {
                    const float t = wd * a.p[j];
                    g = g + t;
                }
                const float m = fmaf(omb1, g, beta1 * a.m[j]);
                const float v = beta2 * a.v[j] + omb2 * g * g;
                a.m[j] = m;
                a.v[j] = v;
                const float pn = a.p[j] * decay - step_size * m / fmaf(sqrtf(v), inv_sqrt_bc2, eps);
                a.p[j] = pn;
                if (averaged) {
                    const float ej = e[j];
                    e[j] = fmaf(w_t, pn - ej, ej);
                }
            }
        }
    }
}
