// The bodies of the small launches that open a training step -- the dropout seed word, the weights' compute-dtype copies, the
// spectral embedding's folded projection, the patch rows and the position/bias rows -- as device functions: ONE body each for the
// stand-alone kernels (spv_misc.hip, spv_patch.hip) and for step_prologue_kernel (spv_misc.hip), which deals its workgroups to these
// roles.  A grid-stride body takes the workgroup's index `bid` among the `nb` workgroups of its role, so a role's workgroup computes
// exactly what the same workgroup of the separate launch computes.
#pragma once
#include "spv_common.h"

constexpr unsigned long long SEED_STEP = 0x9e3779b97f4a7c15ull;   // what one training step adds to the dropout seed word

static __device__ __forceinline__ void st_any(void* base, size_t off, int bf, float v) {
    if (bf) static_cast<bf16_t*>(base)[off] = f2bf(v);
    else static_cast<float*>(base)[off] = v;
}

// One pass over an fp32 weight [rows, cols]: the plain copy in the compute dtype (skipped when plain == nullptr) and the
// transposed copy [cols, ld] (zero beyond rows) -- the two operand layouts the NT GEMMs read.  Run once per weight per
// training step (the copies cannot be cached: see hip_ops._ShadowCache).
template <typename TO>
static __device__ __forceinline__ void weight_shadow_tile(const float* __restrict__ src, TO* __restrict__ plain, TO* __restrict__ tr, int rows,
                                                   int cols, int ld, int bx, int by, float (*tile)[65]) {
    // 32 (rows) x 64 (cols) tile: 16-byte loads along the columns, the transposed copy leaves as 8 consecutive rows per thread
    const int r0 = by * 32, c0 = bx * 64;
    const int t = threadIdx.x;
    const bool vec = (cols & 3) == 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int rl = pass * 16 + (t >> 4), c4 = (t & 15) * 4;
        const int r = r0 + rl, c = c0 + c4;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (r < rows) {
            if (vec && c + 3 < cols) {
                const float4 f = *reinterpret_cast<const float4*>(src + (size_t)r * cols + c);
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                if (plain != nullptr) io<TO>::st4(plain + (size_t)r * cols + c, v);
            } else {
                for (int u = 0; u < 4; ++u)
                    if (c + u < cols) {
                        v[u] = src[(size_t)r * cols + c + u];
                        if (plain != nullptr) io<TO>::st(plain + (size_t)r * cols + c + u, v[u]);
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) tile[rl][c4 + u] = v[u];
    }
    __syncthreads();
    const int cl = t >> 2, r8 = (t & 3) * 8;  // column cl of the tile, rows r8 .. r8 + 7
    const int c = c0 + cl;
    if (c < cols) {
        TO* o = tr + (size_t)c * ld + r0 + r8;
        if (r0 + r8 + 7 < ld && (ld & 7) == 0) {
            float a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = tile[r8 + u][cl]; b[u] = tile[r8 + 4 + u][cl]; }
            io<TO>::st4(o, a);
            io<TO>::st4(o + 4, b);
        } else {
            for (int u = 0; u < 8; ++u)
                if (r0 + r8 + u < ld) io<TO>::st(o + u, tile[r8 + u][cl]);
        }
    }
}

// a row of spv_weight_shadows_multi's device table
struct ShadowTensor { const float* src; void* plain; void* tr; int rows, cols, ld, pad; };

// ---- patch rows: out[row][k] (transposed = 0, leading dim ld >= K) or out[k][row] (transposed = 1, ld >= rows);
// row = b * Np + ih * nW + iw,  k = c * P * P + p * P + q  (spectre.py:130-133 / Conv2d weight order)
static __device__ __forceinline__ void patchify_body(const float* __restrict__ img, void* __restrict__ out, int B, int C, int H, int W, int P,
                                                     int ld, int transposed, int bf, int bid, int nb) {
    const int nH = H / P, nW = W / P, Np = nH * nW, K = C * P * P;
    const int64_t rows = (int64_t)B * Np;
    // transposed == 2: token rows [B][Np + 1][ld], row 0 of every image (the CLS slot) zero -- the layout the token GEMM and the TN
    // weight-gradient GEMM both read as it lies
    const int64_t total = transposed == 1 ? (int64_t)K * ld : (transposed == 2 ? (int64_t)B * (Np + 1) * ld : rows * ld);
    for (int64_t e = (int64_t)bid * blockDim.x + threadIdx.x; e < total; e += (int64_t)nb * blockDim.x) {
        int64_t row;
        int k;
        if (transposed == 1) { k = (int)(e / ld); row = e % ld; }
        else { row = e / ld; k = (int)(e % ld); }
        if (transposed == 2) {
            const int64_t b2 = row / (Np + 1);
            const int t2 = (int)(row % (Np + 1));
            row = t2 == 0 ? rows : b2 * Np + t2 - 1;   // rows = "no such row": zero
        }
        float v = 0.0f;
        if (row < rows && k < K) {
            const int b = (int)(row / Np), n = (int)(row % Np);
            const int ih = n / nW, iw = n % nW;
            const int c = k / (P * P), p = (k / P) % P, q = k % P;
            v = img[(((size_t)b * C + c) * H + ih * P + p) * W + iw * P + q];
        }
        st_any(out, (size_t)e, bf, v);
    }
}

// float NCHW, patch and width multiples of 4, row-major outputs (modes 0 and 2), ld % 4 == 0: one thread per FOUR consecutive k (one
// 16-byte pixel load, one 8/16-byte store).  The element-per-thread form above spends ~10 integer divisions per element: 14.4 us for
// the 3 MB of the CIFAR batch; this form ~3 us.
template <typename T>
static __device__ __forceinline__ void patchify_vec4_body(const float* __restrict__ img, T* __restrict__ out, int B, int C, int H, int W, int P,
                                                          int ld, int token_rows, int bid, int nb) {
    const int nH = H / P, nW = W / P, Np = nH * nW, K = C * P * P;
    const int T1 = token_rows ? Np + 1 : Np;
    const int ld4 = ld >> 2;
    const int64_t total = (int64_t)B * T1 * ld4;
    for (int64_t e = (int64_t)bid * blockDim.x + threadIdx.x; e < total; e += (int64_t)nb * blockDim.x) {
        const int64_t row = e / ld4;
        const int k = (int)(e - row * ld4) * 4;
        const int b = (int)(row / T1), t = (int)(row - (int64_t)b * T1);
        const int n = token_rows ? t - 1 : t;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (n >= 0 && k < K) {
            const int ih = n / nW, iw = n - ih * nW;
            const int c = k / (P * P), r = k - c * P * P, pr = r / P, q = r - pr * P;   // q is a multiple of 4
            const float4 px = *reinterpret_cast<const float4*>(img + (((size_t)b * C + c) * H + ih * P + pr) * W + iw * P + q);
            v[0] = px.x; v[1] = px.y; v[2] = px.z; v[3] = px.w;
        }
        io<T>::st4(out + (size_t)row * ld + k, v);
    }
}

// posbias[t][e] = pos[1 + t][e] + bias[e]
// with cls: one more row in front, out[0][e] = cls[e] + pos[0][e] -- the token GEMM over the zero CLS patch row then writes the CLS token
static __device__ __forceinline__ void posbias_body(const float* __restrict__ pos, const float* __restrict__ bias, const float* __restrict__ cls,
                                                    float* __restrict__ out, int Np, int E, int bid, int nb) {
    const int lead = cls != nullptr ? E : 0;
    const int total = Np * E + lead;
    for (int i = bid * blockDim.x + threadIdx.x; i < total; i += nb * blockDim.x)
        out[i] = i < lead ? cls[i] + pos[i] : pos[E + i - lead] + bias[(i - lead) % E];
}

static __device__ __forceinline__ float rcoef(int u, int v, int p, int q, int P) {
    // Re(rfft2(norm="ortho")) kernel: cos(2 pi (u p + v q) / P) / P      (spectre.py:136)
    return cospif(2.0f * (float)((u * p + v * q) % P) / (float)P) / (float)P;
}

// W_full[e][c,p,q] = sum_{u,v} W[e][c,u,v] fh[u] fw[v] R[(u,v),(p,q)]
static __device__ __forceinline__ void spectral_fold_body(const float* __restrict__ w, const float* __restrict__ fh, const float* __restrict__ fw,
                                                          float* __restrict__ wf, int E, int C, int P, bf16_t* __restrict__ wf_bf, int bid,
                                                          int nb) {
    const int Pv = P / 2 + 1;
    const int total = E * C * P * P;
    for (int i = bid * blockDim.x + threadIdx.x; i < total; i += nb * blockDim.x) {
        const int q = i % P, p = (i / P) % P, c = (i / (P * P)) % C, e = i / (P * P * C);
        const float* wr = w + ((size_t)e * C + c) * P * Pv;
        float a = 0.0f;
        for (int u = 0; u < P; ++u)
            for (int v = 0; v < Pv; ++v) a = fmaf(wr[u * Pv + v] * fh[u] * fw[v], rcoef(u, v, p, q, P), a);
        wf[i] = a;
        if (wf_bf != nullptr) wf_bf[i] = f2bf(a);   // the GEMM operand of a bf16 step: saves the cast launch that followed
    }
}

// the grids of the stand-alone launches (spv_patch.hip), which the prologue's roles repeat
inline int patch_ew_blocks(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 4096); }
