// The update rules beside AdamW on the chunk walk of spv_adamw_core.h: torch.optim.SGD (momentum, dampening, Nesterov, L2 decay;
// maximize off) and torch.optim.Adam (L2 decay, amsgrad off) -- the two other optimizer lines of the reference's script
// (spectre_vit/repl/train.py:197-198, :307).  The table row, the chunk tables, the control block and the weights' moving average are
// the ones AdamW uses; only the body that a workgroup runs on its 2048 elements differs.
#pragma once
#include "spv_adamw_core.h"

// torch.optim.Adam: adamw_chunk with the decay in the gradient (spv_adamw_core.h: L2).  No expression is restated here, so with
// wd == 0 the result is adamw_chunk's bit for bit on the vector and on the scalar walk.
template <bool SCALED, bool EMA = false>
__device__ __forceinline__ void adam_chunk(const AdamTensor a, int n, int off, float lr, float beta1, float beta2, float omb1, float omb2,
                                           float eps, float wd, float bc1, float bc2, const float* __restrict__ step_dev, float gscale,
                                           float* __restrict__ e = nullptr, float ema_w = 0.0f, int ema_warmup = 0, float ema_step = 0.0f) {
    adamw_chunk<SCALED, EMA, true>(a, n, off, lr, beta1, beta2, omb1, omb2, eps, wd, bc1, bc2, step_dev, gscale, e, ema_w, ema_warmup,
                                   ema_step);
}

// The hyper-parameters of one SGD launch, as the kernels take them.  omd = 1 - dampening, formed in double and rounded once by the
// caller.  first: this is the group's first applied step (its step count is 1 after this step's advance): buf = d, torch's
// clone of the first gradient, which dampening does not touch.
struct SgdRule { float lr, momentum, omd, wd; bool nesterov, first; };

// One element of torch.optim.SGD, every line ONE fp32 rounding (no contraction, no fused multiply-add): the vector and the scalar
// walk both call this, so they round alike, and a float32 restatement on the host reproduces the bits (tests/optim_rules_ref.py).
// b is read and written only with momentum != 0.
template <bool SCALED>
__device__ __forceinline__ float sgd_element(float p, float g, float& b, const SgdRule r, float gscale) {
#pragma clang fp contract(off)
    float d = g;
    if (SCALED) d = g * gscale;
    if (r.wd != 0.0f) {
        const float t = r.wd * p;
        d = d + t;
    }
    if (r.momentum != 0.0f) {
        if (r.first) {
            b = d;
        } else {
            const float t1 = r.momentum * b;
            const float t2 = r.omd * d;
            b = t1 + t2;
        }
        if (r.nesterov) {
            const float t = r.momentum * b;
            d = d + t;
        } else {
            d = b;
        }
    }
    const float t = r.lr * d;
    return p - t;
}

// Workgroup `blockIdx.x` updates elements [off, off + 2048) of tensor `a` = {p, g, buf, unused} (n elements): adamw_chunk's walk --
// two float4 per thread where p, g and (with momentum) buf are 16-byte aligned, scalar otherwise and in a tensor's short tail.  With
// momentum == 0 the buf pointer is neither read nor tested.  EMA: adamw_chunk's average, the same expression, fed from the registers
// that hold the new weight; w_t's warm-up reads the step count s of this step.  The walk does not depend on e.
template <bool SCALED, bool EMA = false>
__device__ __forceinline__ void sgd_chunk(const AdamTensor a, int n, int off, const SgdRule r, float s, float gscale,
                                          float* __restrict__ e = nullptr, float ema_w = 0.0f, int ema_warmup = 0) {
#pragma clang fp contract(off)
    const bool mom = r.momentum != 0.0f;
    float w_t = ema_w;
    if (EMA && ema_warmup) w_t = fmaxf(ema_w, 9.0f / (10.0f + s));
    const bool averaged = EMA && e != nullptr;
    const bool e_vec = (reinterpret_cast<uintptr_t>(e) & 15) == 0;
    const bool vec = ((reinterpret_cast<uintptr_t>(a.p) | reinterpret_cast<uintptr_t>(a.g) | (mom ? reinterpret_cast<uintptr_t>(a.m) : 0)) &
                      15) == 0;
    const int base = off + threadIdx.x * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int i = base + h * 1024;
        if (i + 3 < n && vec) {
            float4 p = *reinterpret_cast<const float4*>(a.p + i);
            const float4 g = *reinterpret_cast<const float4*>(a.g + i);
            float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (mom && !r.first) b = *reinterpret_cast<const float4*>(a.m + i);
            float4 ev = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (averaged) {
                if (e_vec) ev = *reinterpret_cast<const float4*>(e + i);
                else ev = make_float4(e[i], e[i + 1], e[i + 2], e[i + 3]);
            }
            float* pp = &p.x; float* bb = &b.x; const float* gg = &g.x; float* ee = &ev.x;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                pp[u] = sgd_element<SCALED>(pp[u], gg[u], bb[u], r, gscale);
                if (EMA) ee[u] = fmaf(w_t, pp[u] - ee[u], ee[u]);
            }
            *reinterpret_cast<float4*>(a.p + i) = p;
            if (mom) *reinterpret_cast<float4*>(a.m + i) = b;
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
                float b = 0.0f;
                if (mom && !r.first) b = a.m[j];
                const float pn = sgd_element<SCALED>(a.p[j], a.g[j], b, r, gscale);
                a.p[j] = pn;
                if (mom) a.m[j] = b;
                if (averaged) {
                    const float ej = e[j];
                    e[j] = fmaf(w_t, pn - ej, ej);
                }
            }
        }
    }
}
