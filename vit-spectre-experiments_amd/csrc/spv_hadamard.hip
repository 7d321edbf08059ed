// spv_hadamard.hip -- Walsh-Hadamard butterflies along the last axis.
// Reference: spectre_vit/models/spectre/hadamar.py -- fwht :12-32 and hadamard_transform :83-112 (natural / Sylvester order,
// optional n^-1/2), fwht_fast :58-80 (each stage writes sum / difference INTERLEAVED, so the output order differs and nothing is
// normalised), LearnableHadamard :115-141 (pad to a power of two, num_blocks x fwht_fast, crop, + residual; its parameters are
// unused: the `* p` is commented out at :136).
#include "spv_common.h"

namespace {

constexpr int HT = 256;

// One workgroup owns `rpw` rows; a row lives in LDS as fp32 (two buffers, ping-pong), one butterfly per thread and stage.
//   mode 0: natural order      stage h: (i, i+h) -> (i, i+h)            (its own transpose)
//   mode 1: fwht_fast          stage h: a=[0,h) b=[h,2h) of a 2h block -> out[2i] = a+b, out[2i+1] = a-b
//   mode 2: fwht_fast^T        stages in reverse; in[2i], in[2i+1] -> out[i] = sum, out[h+i] = difference
template <typename T>
__global__ __launch_bounds__(HT) void fwht_kernel(const T* __restrict__ x, T* __restrict__ y, const T* __restrict__ residual, int rows,
                                                  int n_in, int n, int n_out, int log2n, int mode, int repeat, float scale, int rpw) {
    extern __shared__ float lds[];
    float* buf0 = lds;
    float* buf1 = lds + (size_t)rpw * n;
    const int row0 = blockIdx.x * rpw;
    const int nrows = min(rpw, rows - row0);
    if (nrows <= 0) return;
    for (int e = threadIdx.x; e < nrows * n; e += HT) {
        const int r = e / n, c = e - r * n;
        buf0[e] = c < n_in ? io<T>::ld(x + (size_t)(row0 + r) * n_in + c) : 0.0f;  // F.pad(x, (0, pad))
    }
    __syncthreads();
    float* src = buf0;
    float* dst = buf1;
    const int half = n >> 1;
    for (int rep = 0; rep < repeat; ++rep) {
        for (int s = 0; s < log2n; ++s) {
            const int h = (mode == 2) ? (half >> s) : (1 << s);
            for (int e = threadIdx.x; e < nrows * half; e += HT) {
                const int r = e / half, j = e - r * half;
                const int blk = j / h, i = j - blk * h;
                const float* sp = src + (size_t)r * n + blk * 2 * h;
                float* dp = dst + (size_t)r * n + blk * 2 * h;
                if (mode == 2) {
                    const float u = sp[2 * i], v = sp[2 * i + 1];
                    dp[i] = u + v;
                    dp[h + i] = u - v;
                } else {
                    const float a = sp[i], b = sp[h + i];
                    if (mode == 0) { dp[i] = a + b; dp[h + i] = a - b; }
                    else { dp[2 * i] = a + b; dp[2 * i + 1] = a - b; }
                }
            }
            __syncthreads();
            float* t = src; src = dst; dst = t;
        }
    }
    for (int e = threadIdx.x; e < nrows * n_out; e += HT) {
        const int r = e / n_out, c = e - r * n_out;
        float v = src[(size_t)r * n + c] * scale;                                   // x[..., :orig_dim]
        if (residual) v += io<T>::ld(residual + (size_t)(row0 + r) * n_out + c);   // + residual
        io<T>::st(y + (size_t)(row0 + r) * n_out + c, v);
    }
}

}  // namespace

extern "C" int spv_fwht(const void* x, void* y, const void* residual, int rows, int n_in, int n, int n_out, int mode, int repeat,
                        float scale, int dtype, void* stream) {
    SPV_CHECK(x && y, "spv_fwht: null pointer");
    SPV_CHECK(rows >= 0 && n >= 1 && (n & (n - 1)) == 0 && n <= 16384, "spv_fwht: n = %d must be a power of two <= 16384", n);
    SPV_CHECK(n_in >= 1 && n_in <= n && n_out >= 1 && n_out <= n, "spv_fwht: n_in %d / n_out %d outside 1..%d", n_in, n_out, n);
    SPV_CHECK(mode >= 0 && mode <= 2 && repeat >= 1, "spv_fwht: bad mode %d / repeat %d", mode, repeat);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_fwht: bad dtype %d", dtype);
    if (rows == 0) return 0;
    int log2n = 0;
    while ((1 << log2n) < n) ++log2n;
    const int rpw = n >= 2 * HT ? 1 : (2 * HT) / n;  // keep every thread busy on short rows
    const size_t lds = (size_t)2 * rpw * n * sizeof(float);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(cdiv(rows, rpw));
    if (dtype == SPV_BF16) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fwht_kernel<bf16_t>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipLaunchKernelGGL(fwht_kernel<bf16_t>, grid, dim3(HT), lds, st, (const bf16_t*)x, (bf16_t*)y, (const bf16_t*)residual, rows, n_in, n,
                           n_out, log2n, mode, repeat, scale, rpw);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fwht_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        hipLaunchKernelGGL(fwht_kernel<float>, grid, dim3(HT), lds, st, (const float*)x, (float*)y, (const float*)residual, rows, n_in, n,
                           n_out, log2n, mode, repeat, scale, rpw);
    }
    SPV_LAUNCH_CHECK("spv_fwht");
    return 0;
}

// =====================================================================================================================================
// The 2-D Walsh-Hadamard token mixer  y = crop_{N,D}( H_Np . pad_{Np,Dp}(x) . H_Dp ) . s  (natural order, LearnableHadamard's pad /
// crop convention, hadamar.py:130-139; s = (Np Dp)^-1/2 when normalised).  Symmetric: the same call is its backward.  Because the
// input rows >= N are zero and the output rows >= N are dropped, the token-axis factor is the N x N corner of H_Np, whose entry
// (m, k) is (-1)^popcount(m & k).  spv_hadamard_core.h chooses the kernel.
// =====================================================================================================================================
#include "spv_hadamard_core.h"

namespace {

__device__ __forceinline__ float had_flip(float v, int m, int k) {   // v * H[m][k]
    return __uint_as_float(__float_as_uint(v) ^ ((unsigned)(__builtin_popcount(m & k) & 1) << 31));
}

// in-place natural-order butterflies along the rows of an LDS image [nrows][n] (n = 1 << log2n); every thread of the workgroup calls it
__device__ __forceinline__ void had_rows_lds(float* img, int nrows, int log2n, int nthreads) {
    const int n = 1 << log2n;
    for (int s = 0; s < log2n; ++s) {
        const int h = 1 << s;
        const int total = nrows << (log2n - 1);
        for (int e = threadIdx.x; e < total; e += nthreads) {
            const int r = e >> (log2n - 1), j = e & ((n >> 1) - 1);
            const int i0 = r * n + (((j >> s) << (s + 1)) | (j & (h - 1)));
            const float a = img[i0], b = img[i0 + h];
            img[i0] = a + b;
            img[i0 + h] = a - b;
        }
        __syncthreads();
    }
}

// One workgroup per sample, the image [N][Dp] in LDS as fp32: one read of x, one write of y.  D % 8 == 0, 16-byte accesses.
constexpr int HLT = 512;
template <typename T>
__global__ __launch_bounds__(HLT) void hadamard_lds_kernel(const T* __restrict__ x, T* __restrict__ y, const T* __restrict__ add_in, int N,
                                                           int D, int log2dp, float scale) {
    extern __shared__ float lds[];
    constexpr int EPV = 16 / (int)sizeof(T);
    const int Dp = 1 << log2dp, vpr = Dp / EPV;
    const size_t base = (size_t)blockIdx.x * N * D;
    for (int it = threadIdx.x; it < N * vpr; it += HLT) {
        const int r = it / vpr, c0 = (it - r * vpr) * EPV;
        float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (c0 < D) {   // D is a multiple of 8: a vector lies inside the row or in the pad
            if constexpr (sizeof(T) == 2) {
                const uint4 q = *reinterpret_cast<const uint4*>(x + base + (size_t)r * D + c0);
                v[0] = __uint_as_float(q.x << 16); v[1] = __uint_as_float(q.x & 0xffff0000u);
                v[2] = __uint_as_float(q.y << 16); v[3] = __uint_as_float(q.y & 0xffff0000u);
                v[4] = __uint_as_float(q.z << 16); v[5] = __uint_as_float(q.z & 0xffff0000u);
                v[6] = __uint_as_float(q.w << 16); v[7] = __uint_as_float(q.w & 0xffff0000u);
            } else {
                const float4 q = *reinterpret_cast<const float4*>(x + base + (size_t)r * D + c0);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            }
        }
#pragma unroll
        for (int u = 0; u < EPV; ++u) lds[r * Dp + c0 + u] = v[u];
    }
    __syncthreads();
    had_rows_lds(lds, N, log2dp, HLT);
    // token axis: out[m][c] = sum_k H[m][k] t[k][c], 8 columns per item
    const int gpr = D / 8;
    for (int it = threadIdx.x; it < N * gpr; it += HLT) {
        const int m = it / gpr, c0 = (it - m * gpr) * 8;
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < N; ++k) {
            const float4 a = *reinterpret_cast<const float4*>(lds + k * Dp + c0);
            const float4 b = *reinterpret_cast<const float4*>(lds + k * Dp + c0 + 4);
            acc[0] += had_flip(a.x, m, k); acc[1] += had_flip(a.y, m, k); acc[2] += had_flip(a.z, m, k); acc[3] += had_flip(a.w, m, k);
            acc[4] += had_flip(b.x, m, k); acc[5] += had_flip(b.y, m, k); acc[6] += had_flip(b.z, m, k); acc[7] += had_flip(b.w, m, k);
        }
        const size_t o = base + (size_t)m * D + c0;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] *= scale;
        if (add_in) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += io<T>::ld(add_in + o + u);
        }
        if constexpr (sizeof(T) == 2) {
            uint4 q;
            q.x = pack_bf16x2(acc[0], acc[1]); q.y = pack_bf16x2(acc[2], acc[3]); q.z = pack_bf16x2(acc[4], acc[5]); q.w = pack_bf16x2(acc[6], acc[7]);
            *reinterpret_cast<uint4*>(y + o) = q;
        } else {
            *reinterpret_cast<float4*>(y + o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            *reinterpret_cast<float4*>(y + o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
        }
    }
}

// generic pass 1: rows along D -> fp32 workspace [rows][D] (un-normalised, cropped); any element alignment
template <typename T>
__global__ __launch_bounds__(HT) void hadamard_rows_kernel(const T* __restrict__ x, float* __restrict__ ws, int64_t rows, int D, int log2dp,
                                                           int rpw) {
    extern __shared__ float lds[];
    const int Dp = 1 << log2dp;
    const int64_t row0 = (int64_t)blockIdx.x * rpw;
    const int nrows = (int)(rows - row0 < rpw ? rows - row0 : rpw);
    if (nrows <= 0) return;
    for (int e = threadIdx.x; e < nrows * Dp; e += HT) {
        const int r = e >> log2dp, c = e & (Dp - 1);
        lds[e] = c < D ? io<T>::ld(x + (size_t)(row0 + r) * D + c) : 0.0f;
    }
    __syncthreads();
    had_rows_lds(lds, nrows, log2dp, HT);
    for (int e = threadIdx.x; e < nrows * D; e += HT) {
        const int r = e / D, c = e - r * D;
        ws[(size_t)(row0 + r) * D + c] = lds[r * Dp + c];
    }
}

// generic pass 2: a slab of cs columns of one sample, padded to Np rows, butterflies along the token axis
template <typename T>
__global__ __launch_bounds__(HT) void hadamard_cols_kernel(const float* __restrict__ ws, T* __restrict__ y, const T* __restrict__ add_in, int N,
                                                           int D, int log2np, int log2cs, float scale) {
    extern __shared__ float lds[];
    const int Np = 1 << log2np, cs = 1 << log2cs;
    const int c0 = blockIdx.y * cs;
    const size_t base = (size_t)blockIdx.x * N * D;
    for (int e = threadIdx.x; e < Np * cs; e += HT) {
        const int r = e >> log2cs, c = c0 + (e & (cs - 1));
        lds[e] = (r < N && c < D) ? ws[base + (size_t)r * D + c] : 0.0f;
    }
    __syncthreads();
    for (int s = 0; s < log2np; ++s) {
        const int h = 1 << s;
        for (int e = threadIdx.x; e < (Np >> 1) * cs; e += HT) {
            const int j = e >> log2cs, cc = e & (cs - 1);
            const int i0 = (((j >> s) << (s + 1)) | (j & (h - 1))) * cs + cc;
            const float a = lds[i0], b = lds[i0 + h * cs];
            lds[i0] = a + b;
            lds[i0 + h * cs] = a - b;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < N * cs; e += HT) {
        const int r = e >> log2cs, c = c0 + (e & (cs - 1));
        if (c < D) {
            const size_t o = base + (size_t)r * D + c;
            float v = lds[e] * scale;
            if (add_in) v += io<T>::ld(add_in + o);
            io<T>::st(y + o, v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// Row 0 of  x1 = LayerNorm1(mix(x)) + x : row 0 of H_Np is all ones, so m0 = s . H_D . (sum over tokens of x) -- one pass over the sample
// and ONE D-point transform (D a power of two: no pad along D).  One workgroup of D / 2 threads per sample, thread t owns columns 2t, 2t+1.
template <int D> __device__ __forceinline__ float had_block_sum(float v, float* red, int t) {
    v = wave_sum(v);
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    float a = 0.0f;
#pragma unroll
    for (int w = 0; w < D / 128; ++w) a += red[w];
    return a;
}
template <int D> __device__ __forceinline__ void had_fwht_lds(float* re, int t) {   // D / 2 threads; ends on a barrier
#pragma unroll 1
    for (int h = 1; h < D; h <<= 1) {
        const int i0 = ((t / h) * 2 * h) + (t & (h - 1));
        __syncthreads();
        const float a = re[i0], b = re[i0 + h];
        re[i0] = a + b;
        re[i0 + h] = a - b;
    }
    __syncthreads();
}

template <typename T, int D>
__global__ __launch_bounds__(D / 2) void hadamard_cls_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, T* __restrict__ out, float* __restrict__ m0,
                                                                 float* __restrict__ mean, float* __restrict__ rstd, int N, float scale) {
    __shared__ float re[D], im[D], red[8];
    const int b = blockIdx.x, t = threadIdx.x;
    const T* xs = x + (size_t)b * N * D + 2 * t;
    const float x00 = io<T>::ld(xs), x01 = io<T>::ld(xs + 1);
    constexpr int EPV = 16 / (int)sizeof(T), LPR = D / EPV, RG = (D / 2) / LPR;
    static_assert(RG == 2 || RG == 4, "row groups");
    {
        const int rg = t / LPR, c0 = (t % LPR) * EPV;
        float acc[EPV];
#pragma unroll
        for (int u = 0; u < EPV; ++u) acc[u] = 0.0f;
        const T* xr = x + (size_t)b * N * D + c0;
#pragma unroll 4
        for (int n = rg; n < N; n += RG) {
            if constexpr (sizeof(T) == 2) {
                const uint4 q = *reinterpret_cast<const uint4*>(xr + (size_t)n * D);
                acc[0] += __uint_as_float(q.x << 16); acc[1] += __uint_as_float(q.x & 0xffff0000u);
                acc[2] += __uint_as_float(q.y << 16); acc[3] += __uint_as_float(q.y & 0xffff0000u);
                acc[4] += __uint_as_float(q.z << 16); acc[5] += __uint_as_float(q.z & 0xffff0000u);
                acc[6] += __uint_as_float(q.w << 16); acc[7] += __uint_as_float(q.w & 0xffff0000u);
            } else {
                const float4 q = *reinterpret_cast<const float4*>(xr + (size_t)n * D);
                acc[0] += q.x; acc[1] += q.y; acc[2] += q.z; acc[3] += q.w;
            }
        }
        // row groups 0, 1 into re / im; groups 2, 3 (bf16) added in a second round
        if (rg < 2) {
            float* part = rg == 0 ? re : im;
#pragma unroll
            for (int u = 0; u < EPV; ++u) part[c0 + u] = acc[u];
        }
        __syncthreads();
        if (RG == 4 && rg >= 2) {
            float* p2 = rg == 2 ? re : im;
#pragma unroll
            for (int u = 0; u < EPV; ++u) p2[c0 + u] += acc[u];
        }
        __syncthreads();
    }
    const float s0 = re[2 * t] + im[2 * t], s1 = re[2 * t + 1] + im[2 * t + 1];
    __syncthreads();
    re[2 * t] = s0; re[2 * t + 1] = s1;
    had_fwht_lds<D>(re, t);
    const float a0 = re[2 * t] * scale, a1 = re[2 * t + 1] * scale;
    const float mu = had_block_sum<D>(a0 + a1, red, t) * (1.0f / D);
    const float d0 = a0 - mu, d1 = a1 - mu;
    const float var = had_block_sum<D>(d0 * d0 + d1 * d1, red, t) * (1.0f / D);
    const float rs = rsqrtf(var + 1e-5f);
    m0[(size_t)b * D + 2 * t] = a0; m0[(size_t)b * D + 2 * t + 1] = a1;
    if (t == 0) { mean[b] = mu; rstd[b] = rs; }
    io<T>::st(out + (size_t)b * D + 2 * t, d0 * rs * gamma[2 * t] + beta[2 * t] + x00);
    io<T>::st(out + (size_t)b * D + 2 * t + 1, d1 * rs * gamma[2 * t + 1] + beta[2 * t + 1] + x01);
}

template <typename T, int D>
__global__ __launch_bounds__(D / 2) void hadamard_cls_bwd_kernel(const T* __restrict__ g1, const float* __restrict__ m0,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma, T* __restrict__ dx, float* __restrict__ partials,
                                                                 int N, float scale) {
    __shared__ float re[D], red[8];
    const int b = blockIdx.x, t = threadIdx.x;
    const float mu = mean[b], rs = rstd[b];
    const float g0 = io<T>::ld(g1 + (size_t)b * D + 2 * t), gq = io<T>::ld(g1 + (size_t)b * D + 2 * t + 1);
    const float h0 = (m0[(size_t)b * D + 2 * t] - mu) * rs, h1 = (m0[(size_t)b * D + 2 * t + 1] - mu) * rs;
    float* pp = partials + (size_t)b * 2 * D;   // [2][D]: this sample's dgamma / dbeta contribution
    pp[2 * t] = g0 * h0; pp[2 * t + 1] = gq * h1;
    pp[D + 2 * t] = g0; pp[D + 2 * t + 1] = gq;
    const float q0 = g0 * gamma[2 * t], q1 = gq * gamma[2 * t + 1];
    const float sa = had_block_sum<D>(q0 + q1, red, t) * (1.0f / D);
    const float sb = had_block_sum<D>(q0 * h0 + q1 * h1, red, t) * (1.0f / D);
    re[2 * t] = rs * (q0 - sa - h0 * sb);
    re[2 * t + 1] = rs * (q1 - sa - h1 * sb);
    had_fwht_lds<D>(re, t);
    constexpr int EPV = 16 / (int)sizeof(T), LPR = D / EPV, RG = (D / 2) / LPR;
    const int rg = t / LPR, c0 = (t % LPR) * EPV;
    float v[EPV];
#pragma unroll
    for (int u = 0; u < EPV; ++u) v[u] = re[c0 + u] * scale;
    T* drow = dx + (size_t)b * N * D + c0;
    if (rg == 0) {
        float r0[EPV];
#pragma unroll
        for (int u = 0; u < EPV; ++u) r0[u] = v[u] + io<T>::ld(g1 + (size_t)b * D + c0 + u);
        if constexpr (sizeof(T) == 2) {
            uint4 q;
            q.x = pack_bf16x2(r0[0], r0[1]); q.y = pack_bf16x2(r0[2], r0[3]); q.z = pack_bf16x2(r0[4], r0[5]); q.w = pack_bf16x2(r0[6], r0[7]);
            *reinterpret_cast<uint4*>(drow) = q;
        } else {
            *reinterpret_cast<float4*>(drow) = make_float4(r0[0], r0[1], r0[2], r0[3]);
        }
    }
    if constexpr (sizeof(T) == 2) {
        uint4 q;
        q.x = pack_bf16x2(v[0], v[1]); q.y = pack_bf16x2(v[2], v[3]); q.z = pack_bf16x2(v[4], v[5]); q.w = pack_bf16x2(v[6], v[7]);
#pragma unroll 4
        for (int n = rg == 0 ? RG : rg; n < N; n += RG) *reinterpret_cast<uint4*>(drow + (size_t)n * D) = q;
    } else {
        const float4 q = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll 4
        for (int n = rg == 0 ? RG : rg; n < N; n += RG) *reinterpret_cast<float4*>(drow + (size_t)n * D) = q;
    }
}

// ---------------------------------------------------------------------------------------------------------
// The fused node, bf16, dim 512, 2 <= N <= 65, one 512-thread workgroup per sample, no global scratch:
//   forward   prenorm = mix(x), out = LN(prenorm) gamma + beta + x, mean / rstd per row
//   backward  dx = mix(LN-backward(dout)) + dout, this sample's dgamma / dbeta sums -> partials[b][2][512]
// Plan (both ways):
//   1. the MFMA's B operand goes to LDS as bf16 rows [N][520]: forward x itself (exact); backward e = LN-backward(dout), an fp32 value,
//      as TWO images hi = bf16(e), lo = bf16(e - hi) (the +-1 factor is exact, so the pair keeps ~16 mantissa bits);
//   2. token axis: T = H[:N, :N] . B with v_mfma_f32_32x32x16_bf16, K zero-padded to the step of 16; wave w owns the 64 columns = w mod 8
//      (column = w + 8 lane + 256 tile) as two 32-column tiles, every row tile: acc[3][2] x 16 floats.  The A fragment (+-1 / 0) is formed in registers from popcounts;
//   3. D axis, column bits 3..7 (the lane inside a tile): butterflies across lanes with DPP / ds_swizzle; bit 8 (the tile): registers;
//   4. bits 0..2 cross waves: T goes to LDS as fp32 [N][520] (over the operand images), then one wave per row finishes with an
//      8-point transform in registers and holds the whole row: LayerNorm statistics by wave reduction / the residual add, and the store.
constexpr int HM_D = 512, HM_RS = 520;   // row stride in elements of the LDS images: bf16 rows 1040 B (16-byte pieces, 4 banks apart), fp32
                                         // rows 4 x 520 floats apart = 32 banks between the two half-waves of an accumulator store
typedef __attribute__((ext_vector_type(4))) unsigned had_u32x4;

template <int XM> __device__ __forceinline__ float had_swz(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (XM << 10) | 0x1F));
}

template <int BWD>
__global__ __launch_bounds__(512) void hadamard_mfma_kernel(const bf16_t* __restrict__ xin,      // fwd: x          bwd: dout
                                                            bf16_t* __restrict__ prenorm,         // fwd: written    bwd: read
                                                            bf16_t* __restrict__ yout,            // fwd: out        bwd: dx
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ partials,
                                                            int N, float scale) {
    extern __shared__ float lds[];
    bf16_t* img = reinterpret_cast<bf16_t*>(lds);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g = lane >> 5, c = lane & 31;
    const size_t base = (size_t)blockIdx.x * N * HM_D;
    const int lo_off = N * HM_RS;   // elements from the hi image to the lo image (backward)

    // ---- 1. operand images
    if constexpr (!BWD) {
        for (int it = t; it < N * 64; it += 512) {
            const int r = it >> 6, v = it & 63;
            *reinterpret_cast<uint4*>(img + r * HM_RS + v * 8) = *reinterpret_cast<const uint4*>(xin + base + (size_t)r * HM_D + v * 8);
        }
    } else {
        float* red = lds + (size_t)N * HM_RS;   // [8][512] floats behind the images
        float gm[8], dg[8], db[8];
        {
            const float4 a = *reinterpret_cast<const float4*>(gamma + lane * 8), b4 = *reinterpret_cast<const float4*>(gamma + lane * 8 + 4);
            gm[0] = a.x; gm[1] = a.y; gm[2] = a.z; gm[3] = a.w; gm[4] = b4.x; gm[5] = b4.y; gm[6] = b4.z; gm[7] = b4.w;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { dg[u] = 0.0f; db[u] = 0.0f; }
        for (int r = wave; r < N; r += 8) {
            const size_t o = base + (size_t)r * HM_D + lane * 8;
            const uint4 qd = *reinterpret_cast<const uint4*>(xin + o), qp = *reinterpret_cast<const uint4*>(prenorm + o);
            const float mu = mean[(size_t)blockIdx.x * N + r], rs = rstd[(size_t)blockIdx.x * N + r];
            float d[8], h[8], q[8];
            d[0] = __uint_as_float(qd.x << 16); d[1] = __uint_as_float(qd.x & 0xffff0000u);
            d[2] = __uint_as_float(qd.y << 16); d[3] = __uint_as_float(qd.y & 0xffff0000u);
            d[4] = __uint_as_float(qd.z << 16); d[5] = __uint_as_float(qd.z & 0xffff0000u);
            d[6] = __uint_as_float(qd.w << 16); d[7] = __uint_as_float(qd.w & 0xffff0000u);
            h[0] = __uint_as_float(qp.x << 16); h[1] = __uint_as_float(qp.x & 0xffff0000u);
            h[2] = __uint_as_float(qp.y << 16); h[3] = __uint_as_float(qp.y & 0xffff0000u);
            h[4] = __uint_as_float(qp.z << 16); h[5] = __uint_as_float(qp.z & 0xffff0000u);
            h[6] = __uint_as_float(qp.w << 16); h[7] = __uint_as_float(qp.w & 0xffff0000u);
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                h[u] = (h[u] - mu) * rs;
                q[u] = d[u] * gm[u];
                s1 += q[u];
                s2 += q[u] * h[u];
                dg[u] += d[u] * h[u];
                db[u] += d[u];
            }
            const float sa = wave_sum(s1) * (1.0f / HM_D), sb = wave_sum(s2) * (1.0f / HM_D);
            float hi[8], lo[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float e = rs * (q[u] - sa - h[u] * sb);
                hi[u] = bf2f(f2bf(e));
                lo[u] = e - hi[u];
            }
            uint4 qh, ql;
            qh.x = pack_bf16x2(hi[0], hi[1]); qh.y = pack_bf16x2(hi[2], hi[3]); qh.z = pack_bf16x2(hi[4], hi[5]); qh.w = pack_bf16x2(hi[6], hi[7]);
            ql.x = pack_bf16x2(lo[0], lo[1]); ql.y = pack_bf16x2(lo[2], lo[3]); ql.z = pack_bf16x2(lo[4], lo[5]); ql.w = pack_bf16x2(lo[6], lo[7]);
            *reinterpret_cast<uint4*>(img + r * HM_RS + lane * 8) = qh;
            *reinterpret_cast<uint4*>(img + lo_off + r * HM_RS + lane * 8) = ql;
        }
        // the sample's column sums: waves in a fixed order, dgamma then dbeta through the same 16 KB
        float* pp = partials + (size_t)blockIdx.x * 2 * HM_D;
#pragma unroll
        for (int u = 0; u < 8; ++u) red[wave * HM_D + lane * 8 + u] = dg[u];
        __syncthreads();
        {
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < 8; ++w) s += red[w * HM_D + t];
            pp[t] = s;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) red[wave * HM_D + lane * 8 + u] = db[u];
        __syncthreads();
        {
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < 8; ++w) s += red[w * HM_D + t];
            pp[HM_D + t] = s;
        }
    }
    __syncthreads();

    // ---- 2. token axis on the MFMA
    const int MT = (N + 31) >> 5, KS = (N + 15) >> 4;
    f32x16 acc[3][2];
#pragma unroll
    for (int mt = 0; mt < 3; ++mt)
#pragma unroll
        for (int tl = 0; tl < 2; ++tl)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][tl][r] = 0.0f;
    for (int ks = 0; ks < KS; ++ks) {
        const int k0 = ks * 16 + 8 * g;
        bf16x8 bh[2], bl[2];
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            const int col = wave + 8 * (tl * 32 + c);   // column bits 0..2 = wave, 3..7 = lane, 8 = tile
            unsigned h[8], l[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool in = k0 + e < N;                       // K padding: rows >= N are not in LDS
                const int off = (in ? k0 + e : 0) * HM_RS + col;
                h[e] = in ? img[off] : 0u;
                l[e] = (BWD && in) ? img[lo_off + off] : 0u;
            }
            had_u32x4 ph = {h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
            bh[tl] = __builtin_bit_cast(bf16x8, ph);
            if constexpr (BWD) {
                had_u32x4 pl = {l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16)};
                bl[tl] = __builtin_bit_cast(bf16x8, pl);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 3; ++mt) {
            if (mt < MT) {
                const int m = mt * 32 + c;
                unsigned a[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = k0 + e;
                    a[e] = (m < N && k < N) ? (0x3F80u | ((unsigned)(__builtin_popcount(m & k) & 1) << 15)) : 0u;   // +-1.0 in bf16
                }
                had_u32x4 pa = {a[0] | (a[1] << 16), a[2] | (a[3] << 16), a[4] | (a[5] << 16), a[6] | (a[7] << 16)};
                const bf16x8 af = __builtin_bit_cast(bf16x8, pa);
#pragma unroll
                for (int tl = 0; tl < 2; ++tl) {
                    acc[mt][tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bh[tl], acc[mt][tl], 0, 0, 0);
                    if constexpr (BWD) acc[mt][tl] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bl[tl], acc[mt][tl], 0, 0, 0);
                }
            }
        }
    }

    // ---- 3. D axis inside the wave: column bits 3..7 across lanes, bit 8 between the two tiles
    const float sg0 = (c & 1) ? -1.0f : 1.0f, sg1 = (c & 2) ? -1.0f : 1.0f, sg2 = (c & 4) ? -1.0f : 1.0f, sg3 = (c & 8) ? -1.0f : 1.0f,
                sg4 = (c & 16) ? -1.0f : 1.0f;
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        if (mt < MT) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma unroll
                for (int tl = 0; tl < 2; ++tl) {
                    float v = acc[mt][tl][r];
                    v = fmaf(sg0, v, dpp_mov<0xB1>(v));    // lane ^ 1: the upper lane of a pair gets partner - own
                    v = fmaf(sg1, v, dpp_mov<0x4E>(v));    // lane ^ 2
                    v = fmaf(sg2, v, had_swz<4>(v));       // lane ^ 4
                    v = fmaf(sg3, v, dpp_mov<0x128>(v));   // row_ror:8 of a 16-lane row = lane ^ 8
                    v = fmaf(sg4, v, had_swz<16>(v));      // lane ^ 16 (inside the 32-lane half that shares the rows)
                    acc[mt][tl][r] = v;
                }
                const float a = acc[mt][0][r], b = acc[mt][1][r];
                acc[mt][0][r] = a + b;
                acc[mt][1][r] = a - b;
            }
        }
    }

    // ---- 4. through LDS for the bits that cross waves
    __syncthreads();   // every wave is done reading the operand images
    float* tl_img = lds;
#pragma unroll
    for (int mt = 0; mt < 3; ++mt) {
        if (mt < MT) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
                if (m < N) {
                    tl_img[m * HM_RS + wave * 64 + c] = acc[mt][0][r];
                    tl_img[m * HM_RS + wave * 64 + 32 + c] = acc[mt][1][r];
                }
            }
        }
    }
    __syncthreads();
    // slot q * 64 + lane of a row holds column 8 lane + q (wave q produced it): a lane owns eight adjacent columns, 16 bytes
    float gq[8], bq[8];
    if constexpr (!BWD) {
        const float4 g0 = *reinterpret_cast<const float4*>(gamma + lane * 8), g1 = *reinterpret_cast<const float4*>(gamma + lane * 8 + 4);
        const float4 b0 = *reinterpret_cast<const float4*>(beta + lane * 8), b1 = *reinterpret_cast<const float4*>(beta + lane * 8 + 4);
        gq[0] = g0.x; gq[1] = g0.y; gq[2] = g0.z; gq[3] = g0.w; gq[4] = g1.x; gq[5] = g1.y; gq[6] = g1.z; gq[7] = g1.w;
        bq[0] = b0.x; bq[1] = b0.y; bq[2] = b0.z; bq[3] = b0.w; bq[4] = b1.x; bq[5] = b1.y; bq[6] = b1.z; bq[7] = b1.w;
    }
    for (int r = wave; r < N; r += 8) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = tl_img[r * HM_RS + q * 64 + lane];
#pragma unroll
        for (int h = 1; h < 8; h <<= 1) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (!(q & h)) {
                    const float a = v[q], b = v[q + h];
                    v[q] = a + b;
                    v[q + h] = a - b;
                }
            }
        }
        const size_t o = base + (size_t)r * HM_D + lane * 8;
        const uint4 qx = *reinterpret_cast<const uint4*>(xin + o);   // the residual: x (forward) / dout (backward)
        float xr[8];
        xr[0] = __uint_as_float(qx.x << 16); xr[1] = __uint_as_float(qx.x & 0xffff0000u);
        xr[2] = __uint_as_float(qx.y << 16); xr[3] = __uint_as_float(qx.y & 0xffff0000u);
        xr[4] = __uint_as_float(qx.z << 16); xr[5] = __uint_as_float(qx.z & 0xffff0000u);
        xr[6] = __uint_as_float(qx.w << 16); xr[7] = __uint_as_float(qx.w & 0xffff0000u);
        float w[8];
        if constexpr (!BWD) {
            uint4 qp;
            qp.x = pack_bf16x2(v[0] * scale, v[1] * scale); qp.y = pack_bf16x2(v[2] * scale, v[3] * scale);
            qp.z = pack_bf16x2(v[4] * scale, v[5] * scale); qp.w = pack_bf16x2(v[6] * scale, v[7] * scale);
            *reinterpret_cast<uint4*>(prenorm + o) = qp;
            // the statistics are those of the STORED prenorm: the backward re-forms xhat from it
            v[0] = __uint_as_float(qp.x << 16); v[1] = __uint_as_float(qp.x & 0xffff0000u);
            v[2] = __uint_as_float(qp.y << 16); v[3] = __uint_as_float(qp.y & 0xffff0000u);
            v[4] = __uint_as_float(qp.z << 16); v[5] = __uint_as_float(qp.z & 0xffff0000u);
            v[6] = __uint_as_float(qp.w << 16); v[7] = __uint_as_float(qp.w & 0xffff0000u);
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q) s += v[q];
            const float mu = wave_sum(s) * (1.0f / HM_D);
            float s2 = 0.0f;
#pragma unroll
            for (int q = 0; q < 8; ++q) { const float d = v[q] - mu; s2 += d * d; }
            const float rs = rsqrtf(wave_sum(s2) * (1.0f / HM_D) + 1e-5f);
            if (lane == 0) { mean[(size_t)blockIdx.x * N + r] = mu; rstd[(size_t)blockIdx.x * N + r] = rs; }
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = (v[q] - mu) * rs * gq[q] + bq[q] + xr[q];
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = v[q] * scale + xr[q];
        }
        uint4 qo;
        qo.x = pack_bf16x2(w[0], w[1]); qo.y = pack_bf16x2(w[2], w[3]); qo.z = pack_bf16x2(w[4], w[5]); qo.w = pack_bf16x2(w[6], w[7]);
        *reinterpret_cast<uint4*>(yout + o) = qo;
    }
}

const char* hadamard_refusal(int code) {
    switch (code) {
        case HADAMARD_REFUSE_EMPTY: return "empty";
        case HADAMARD_REFUSE_DTYPE: return "bad dtype";
        case HADAMARD_REFUSE_DIM: return "dim pads beyond 16384";
        case HADAMARD_REFUSE_TOKENS: return "tokens pad beyond 32768";
        case HADAMARD_REFUSE_WORKSPACE: return "workspace required";
    }
    return "unserved";
}

bool had_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

template <typename K> void had_allow_lds(K kernel) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

}  // namespace

static_assert(HADAMARD_ONE_KERNEL == SPV_HADAMARD_ONE_KERNEL && HADAMARD_GENERIC == SPV_HADAMARD_GENERIC &&
              HADAMARD_REFUSE_EMPTY == SPV_HADAMARD_REFUSE_EMPTY && HADAMARD_REFUSE_DTYPE == SPV_HADAMARD_REFUSE_DTYPE &&
              HADAMARD_REFUSE_DIM == SPV_HADAMARD_REFUSE_DIM && HADAMARD_REFUSE_TOKENS == SPV_HADAMARD_REFUSE_TOKENS &&
              HADAMARD_REFUSE_WORKSPACE == SPV_HADAMARD_REFUSE_WORKSPACE, "spv.h and spv_hadamard_core.h name the same codes");

extern "C" int spv_hadamard_path(int dtype, int tokens, int dim, int has_workspace) {
    return hadamard_select(dtype, tokens, dim, has_workspace != 0).path;
}

extern "C" int64_t spv_hadamard_workspace_floats(int batch, int tokens, int dim) { return hadamard_workspace_floats(batch, tokens, dim); }

extern "C" int spv_hadamard_mix(const void* x, void* y, const void* add_in, int batch, int tokens, int dim, float scale, int dtype,
                                float* workspace, void* stream) {
    SPV_CHECK(batch > 0, "spv_hadamard_mix: empty");
    const HadamardPlan p = hadamard_select(dtype, tokens, dim, workspace != nullptr);
    SPV_CHECK(p.path > 0, "spv_hadamard_mix: %s (tokens=%d dim=%d dtype=%d)", hadamard_refusal(p.path), tokens, dim, dtype);
    SPV_CHECK(x && y, "spv_hadamard_mix: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int log2dp = hadamard_log2(p.dp), log2np = hadamard_log2(p.np);
    if (p.path == HADAMARD_ONE_KERNEL) {
        SPV_CHECK(had_aligned16(x, y, add_in), "spv_hadamard_mix: x, y and add_in must be 16-byte aligned for tokens=%d dim=%d", tokens, dim);
        if (dtype == SPV_BF16) {
            had_allow_lds(&hadamard_lds_kernel<bf16_t>);
            hipLaunchKernelGGL(hadamard_lds_kernel<bf16_t>, dim3(batch), dim3(HLT), p.lds, st, (const bf16_t*)x, (bf16_t*)y, (const bf16_t*)add_in,
                               tokens, dim, log2dp, scale);
        } else {
            had_allow_lds(&hadamard_lds_kernel<float>);
            hipLaunchKernelGGL(hadamard_lds_kernel<float>, dim3(batch), dim3(HLT), p.lds, st, (const float*)x, (float*)y, (const float*)add_in,
                               tokens, dim, log2dp, scale);
        }
        SPV_LAUNCH_CHECK("spv_hadamard_mix(one kernel)");
        return 0;
    }
    const int64_t rows = (int64_t)batch * tokens;
    const int64_t groups = (rows + p.rpw - 1) / p.rpw;
    SPV_CHECK(groups <= 0x7fffffff, "spv_hadamard_mix: too many rows");
    const size_t lds1 = (size_t)p.rpw * p.dp * 4, lds2 = (size_t)p.np * p.cs * 4;
    const dim3 grid2(batch, cdiv(dim, p.cs));
    const int log2cs = hadamard_log2(p.cs);
    if (dtype == SPV_BF16) {
        had_allow_lds(&hadamard_rows_kernel<bf16_t>);
        had_allow_lds(&hadamard_cols_kernel<bf16_t>);
        hipLaunchKernelGGL(hadamard_rows_kernel<bf16_t>, dim3((unsigned)groups), dim3(HT), lds1, st, (const bf16_t*)x, workspace, rows, dim, log2dp,
                           p.rpw);
        SPV_LAUNCH_CHECK("spv_hadamard_mix(rows)");
        hipLaunchKernelGGL(hadamard_cols_kernel<bf16_t>, grid2, dim3(HT), lds2, st, (const float*)workspace, (bf16_t*)y, (const bf16_t*)add_in,
                           tokens, dim, log2np, log2cs, scale);
    } else {
        had_allow_lds(&hadamard_rows_kernel<float>);
        had_allow_lds(&hadamard_cols_kernel<float>);
        hipLaunchKernelGGL(hadamard_rows_kernel<float>, dim3((unsigned)groups), dim3(HT), lds1, st, (const float*)x, workspace, rows, dim, log2dp,
                           p.rpw);
        SPV_LAUNCH_CHECK("spv_hadamard_mix(rows)");
        hipLaunchKernelGGL(hadamard_cols_kernel<float>, grid2, dim3(HT), lds2, st, (const float*)workspace, (float*)y, (const float*)add_in, tokens,
                           dim, log2np, log2cs, scale);
    }
    SPV_LAUNCH_CHECK("spv_hadamard_mix(columns)");
    return 0;
}

extern "C" int spv_hadamard_ln_supported(int tokens, int dim, int dtype) { return hadamard_ln_supported(tokens, dim, dtype); }

extern "C" int spv_hadamard_ln_fwd(const void* x, void* prenorm, void* out, const float* gamma, const float* beta, float* mean, float* rstd,
                                   float scale, int batch, int tokens, int dim, int dtype, void* stream) {
    SPV_CHECK(hadamard_ln_supported(tokens, dim, dtype), "spv_hadamard_ln_fwd: unsupported tokens=%d dim=%d dtype=%d", tokens, dim, dtype);
    SPV_CHECK(batch > 0, "spv_hadamard_ln_fwd: empty batch");
    SPV_CHECK(x && prenorm && out && gamma && beta && mean && rstd, "spv_hadamard_ln_fwd: null pointer");
    SPV_CHECK(had_aligned16(x, prenorm, out) && had_aligned16(gamma, beta), "spv_hadamard_ln_fwd: x, prenorm, out, gamma and beta must be 16-byte aligned");
    had_allow_lds(&hadamard_mfma_kernel<0>);
    const size_t lds = (size_t)tokens * HM_RS * 4;
    hipLaunchKernelGGL(hadamard_mfma_kernel<0>, dim3(batch), dim3(512), lds, static_cast<hipStream_t>(stream), (const bf16_t*)x, (bf16_t*)prenorm,
                       (bf16_t*)out, gamma, beta, mean, rstd, (float*)nullptr, tokens, scale);
    SPV_LAUNCH_CHECK("spv_hadamard_ln_fwd");
    return 0;
}

extern "C" int spv_hadamard_ln_bwd(const void* dout, const void* prenorm, const float* mean, const float* rstd, const float* gamma, void* dx,
                                   float* dgamma, float* dbeta, float* partials, float scale, int batch, int tokens, int dim, int dtype,
                                   void* stream) {
    SPV_CHECK(hadamard_ln_supported(tokens, dim, dtype), "spv_hadamard_ln_bwd: unsupported tokens=%d dim=%d dtype=%d", tokens, dim, dtype);
    SPV_CHECK(batch > 0, "spv_hadamard_ln_bwd: empty batch");
    SPV_CHECK(dout && prenorm && mean && rstd && gamma && dx && partials, "spv_hadamard_ln_bwd: null pointer");
    SPV_CHECK((dgamma == nullptr) == (dbeta == nullptr), "spv_hadamard_ln_bwd: dgamma and dbeta go together");
    SPV_CHECK(had_aligned16(dout, prenorm, dx, gamma), "spv_hadamard_ln_bwd: dout, prenorm, dx and gamma must be 16-byte aligned");
    had_allow_lds(&hadamard_mfma_kernel<1>);
    const size_t lds = (size_t)tokens * HM_RS * 4 + 8 * HM_D * 4;
    hipLaunchKernelGGL(hadamard_mfma_kernel<1>, dim3(batch), dim3(512), lds, static_cast<hipStream_t>(stream), (const bf16_t*)dout,
                       (bf16_t*)const_cast<void*>(prenorm), (bf16_t*)dx, gamma, (const float*)nullptr, const_cast<float*>(mean),
                       const_cast<float*>(rstd), partials, tokens, scale);
    SPV_LAUNCH_CHECK("spv_hadamard_ln_bwd");
    if (dgamma) {
        spv_fold_job job = {partials, {dgamma, dbeta, nullptr, nullptr, nullptr}, batch, 2, dim};
        return spv_fold_multi(&job, 1, stream);
    }
    return 0;
}

extern "C" int spv_hadamard_cls_supported(int tokens, int dim, int dtype) { return hadamard_cls_supported(tokens, dim, dtype); }

extern "C" int spv_hadamard_cls_fwd(const void* x, const float* gamma, const float* beta, void* out, float* m0, float* mean, float* rstd,
                                    float scale, int batch, int tokens, int dim, int dtype, void* stream) {
    SPV_CHECK(hadamard_cls_supported(tokens, dim, dtype), "spv_hadamard_cls_fwd: unsupported tokens=%d dim=%d dtype=%d", tokens, dim, dtype);
    SPV_CHECK(batch > 0, "spv_hadamard_cls_fwd: empty batch");
    SPV_CHECK(x && gamma && beta && out && m0 && mean && rstd, "spv_hadamard_cls_fwd: null pointer");
    SPV_CHECK(had_aligned16(x, out), "spv_hadamard_cls_fwd: x and out must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SPV_HCLS_F(TT, DD) hipLaunchKernelGGL((hadamard_cls_fwd_kernel<TT, DD>), dim3(batch), dim3(DD / 2), 0, st, (const TT*)x, gamma, beta, (TT*)out, m0, mean, rstd, tokens, scale)
    if (dtype == SPV_BF16) { if (dim == 256) SPV_HCLS_F(bf16_t, 256); else if (dim == 512) SPV_HCLS_F(bf16_t, 512); else SPV_HCLS_F(bf16_t, 1024); }
    else { if (dim == 256) SPV_HCLS_F(float, 256); else if (dim == 512) SPV_HCLS_F(float, 512); else SPV_HCLS_F(float, 1024); }
#undef SPV_HCLS_F
    SPV_LAUNCH_CHECK("spv_hadamard_cls_fwd");
    return 0;
}

extern "C" int spv_hadamard_cls_bwd(const void* g1, const float* m0, const float* mean, const float* rstd, const float* gamma, void* dx,
                                    float* partials, float scale, int batch, int tokens, int dim, int dtype, void* stream) {
    SPV_CHECK(hadamard_cls_supported(tokens, dim, dtype), "spv_hadamard_cls_bwd: unsupported tokens=%d dim=%d dtype=%d", tokens, dim, dtype);
    SPV_CHECK(batch > 0, "spv_hadamard_cls_bwd: empty batch");
    SPV_CHECK(g1 && m0 && mean && rstd && gamma && dx && partials, "spv_hadamard_cls_bwd: null pointer");
    SPV_CHECK(had_aligned16(dx), "spv_hadamard_cls_bwd: dx must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SPV_HCLS_B(TT, DD) hipLaunchKernelGGL((hadamard_cls_bwd_kernel<TT, DD>), dim3(batch), dim3(DD / 2), 0, st, (const TT*)g1, m0, mean, rstd, gamma, (TT*)dx, partials, tokens, scale)
    if (dtype == SPV_BF16) { if (dim == 256) SPV_HCLS_B(bf16_t, 256); else if (dim == 512) SPV_HCLS_B(bf16_t, 512); else SPV_HCLS_B(bf16_t, 1024); }
    else { if (dim == 256) SPV_HCLS_B(float, 256); else if (dim == 512) SPV_HCLS_B(float, 512); else SPV_HCLS_B(float, 1024); }
#undef SPV_HCLS_B
    SPV_LAUNCH_CHECK("spv_hadamard_cls_bwd");
    return 0;
}
