// SpectreBranch feature extractor (reference spectre_vit/models/spectre_branch/spectre_branch.py:122-173): the log-magnitude image
// spectrum, the chain of valid 3x3 convolutions and the adaptive token pooling of each stage's map.
//
// Layout.  Every stage map is channels-last, (B, H, W, C) with no padding, so position m = (b, h, w) is one GEMM row and the
// pooling windows over the flattened H*W map are runs of rows.  The convolution is an im2col GEMM on the library's MFMA kernel
// (spv_gemm_nt): a gather kernel writes the (position, K) operand with K ordered (c, ky, kx) -- the order of the PyTorch weight
// [Cout][Cin][3][3], so the forward weight operand is the parameter itself reshaped (K zero-padded to 16 bytes) and the weight
// gradient comes out in the parameter's own layout.  All reductions run in a fixed order (split-K through the GEMM's workspace
// and reduce kernel): deterministic, no float atomics.
#include "spv_common.h"

namespace {

inline int round8(int v) { return (v + 7) / 8 * 8; }

// ---------------------------------------------------------------- log1p(|rfft2(img)|)
// One workgroup per (sample, channel) plane: the row DFT (length W, Wf = W/2+1 bins) into LDS, then the column DFT (length H).
// Twiddles come from an exact integer phase (k * n mod N) and a table built in double precision.
template <typename T>
__global__ void __launch_bounds__(256) spectrum_kernel(const float* __restrict__ img, T* __restrict__ out, int C, int H, int W) {
    extern __shared__ float lds[];
    const int Wf = W / 2 + 1;
    float* cw = lds;            // cos(2 pi k / W), sin(2 pi k / W)
    float* sw = cw + W;
    float* ch = sw + W;         // the same over H
    float* sh = ch + H;
    float* rr = sh + H;         // row transform, (H, Wf)
    float* ri = rr + H * Wf;
    const int plane = blockIdx.x;
    const int b = plane / C, c = plane % C;
    const float* x = img + (int64_t)plane * H * W;
    for (int k = threadIdx.x; k < W; k += blockDim.x) {
        double s, co;
        sincospi(2.0 * k / W, &s, &co);
        cw[k] = (float)co;
        sw[k] = (float)s;
    }
    for (int k = threadIdx.x; k < H; k += blockDim.x) {
        double s, co;
        sincospi(2.0 * k / H, &s, &co);
        ch[k] = (float)co;
        sh[k] = (float)s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < H * Wf; i += blockDim.x) {
        const int h = i / Wf, v = i % Wf;
        const float* row = x + (int64_t)h * W;
        float re = 0.0f, im = 0.0f;
        int ph = 0;
        for (int w = 0; w < W; ++w) {
            const float a = row[w];
            re += a * cw[ph];
            im -= a * sw[ph];
            ph += v;
            if (ph >= W) ph -= W;
        }
        rr[i] = re;
        ri[i] = im;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < H * Wf; i += blockDim.x) {
        const int u = i / Wf, v = i % Wf;
        float re = 0.0f, im = 0.0f;
        int ph = 0;
        for (int h = 0; h < H; ++h) {
            const float a = rr[h * Wf + v], bb = ri[h * Wf + v];
            const float co = ch[ph], s = sh[ph];
            re += a * co + bb * s;
            im += bb * co - a * s;
            ph += u;
            if (ph >= H) ph -= H;
        }
        io<T>::st(out + (((int64_t)b * H + u) * Wf + v) * C + c, log1pf(hypotf(re, im)));
    }
}

// ---------------------------------------------------------------- im2col gathers
// forward / weight-gradient operand: cols[m][k] = x[b, ho + ky, wo + kx, c], m = (b, ho, wo), k = (c, ky, kx) < 9 Cin, zero for
// k in [9 Cin, ldk).  transposed: colsT[k][m] for k < 9 Cin, m < ldm (zero for m >= M).
template <typename T, bool TRANS>
__global__ void __launch_bounds__(256) im2col_kernel(const T* __restrict__ x, T* __restrict__ cols, int H, int W, int Cin, int64_t M,
                                                     int64_t ld, int64_t total) {
    const int Ho = H - 2, Wo = W - 2;
    const int K = 9 * Cin;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t m;
        int k;
        if (TRANS) {
            k = (int)(i / ld);
            m = i % ld;
        } else {
            m = i / ld;
            k = (int)(i % ld);
        }
        float v = 0.0f;
        if (k < K && m < M) {
            const int c = k / 9, r = k % 9, ky = r / 3, kx = r % 3;
            const int wo = (int)(m % Wo);
            const int64_t t = m / Wo;
            const int ho = (int)(t % Ho);
            const int64_t b = t / Ho;
            v = io<T>::ld(x + ((b * H + ho + ky) * W + wo + kx) * Cin + c);
        }
        io<T>::st(cols + i, v);
    }
}

// data-gradient operand (the full correlation): dcols[m][k] = dy[b, h - ky, w - kx, co], m = (b, h, w) over the INPUT map,
// k = (co, ky, kx) < 9 Cout, zero where (h - ky, w - kx) falls off the output map and for k in [9 Cout, ldk)
template <typename T>
__global__ void __launch_bounds__(256) dcols_kernel(const T* __restrict__ dy, T* __restrict__ dcols, int H, int W, int Cout, int ldk,
                                                    int64_t total) {
    const int Ho = H - 2, Wo = W - 2;
    const int K = 9 * Cout;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / ldk;
        const int k = (int)(i % ldk);
        float v = 0.0f;
        if (k < K) {
            const int co = k / 9, r = k % 9, ky = r / 3, kx = r % 3;
            const int w = (int)(m % W);
            const int64_t t = m / W;
            const int h = (int)(t % H);
            const int64_t b = t / H;
            const int ho = h - ky, wo = w - kx;
            if (ho >= 0 && ho < Ho && wo >= 0 && wo < Wo) v = io<T>::ld(dy + ((b * Ho + ho) * Wo + wo) * Cout + co);
        }
        io<T>::st(dcols + i, v);
    }
}

// dyT[co][m] = dy[m][co] (zero for m in [M, ldm))
template <typename T>
__global__ void __launch_bounds__(256) transpose_rows_kernel(const T* __restrict__ dy, T* __restrict__ dyt, int64_t M, int C, int64_t ldm,
                                                             int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int co = (int)(i / ldm);
        const int64_t m = i % ldm;
        io<T>::st(dyt + i, m < M ? io<T>::ld(dy + m * C + co) : 0.0f);
    }
}

// ---------------------------------------------------------------- AdaptiveAvgPool1d over the flattened map, token-major
// window i of T over L: [floor(i L / T), ceil((i + 1) L / T)); position l lies in windows floor(l T / L) .. floor(((l + 1) T - 1) / L)
__device__ __forceinline__ int win_start(int i, int L, int T) { return (int)(((int64_t)i * L) / T); }
__device__ __forceinline__ int win_end(int i, int L, int T) { return (int)(((int64_t)(i + 1) * L + T - 1) / T); }

template <typename T>
__global__ void __launch_bounds__(256) pool_fwd_kernel(const T* __restrict__ y, T* __restrict__ out, int L, int C, int Tk, int ldo,
                                                       int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % ldo);
        const int64_t bt = i / ldo;
        const int t = (int)(bt % Tk);
        const int64_t b = bt / Tk;
        float v = 0.0f;
        if (c < C) {
            const int s = win_start(t, L, Tk), e = win_end(t, L, Tk);
            const T* p = y + (b * L + s) * C + c;
            for (int l = s; l < e; ++l, p += C) v += io<T>::ld(p);
            v /= (float)(e - s);
        }
        io<T>::st(out + i, v);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) pool_bwd_kernel(const T* __restrict__ dout, int ldo, const T* __restrict__ add, T* __restrict__ dy,
                                                       int L, int C, int Tk, int64_t total) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t bl = i / C;
        const int l = (int)(bl % L);
        const int64_t b = bl / L;
        const int lo = (int)(((int64_t)l * Tk) / L);
        const int hi = min(Tk - 1, (int)((((int64_t)l + 1) * Tk - 1) / L));
        float v = 0.0f;
        for (int t = lo; t <= hi; ++t) {
            const int s = win_start(t, L, Tk), e = win_end(t, L, Tk);
            if (l >= s && l < e) v += io<T>::ld(dout + (b * Tk + t) * ldo + c) / (float)(e - s);
        }
        if (add) v += io<T>::ld(add + i);
        io<T>::st(dy + i, v);
    }
}

inline int grid_for(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 65536); }

}  // namespace

extern "C" int spv_spectrum_floats(int H, int W) { return 2 * W + 2 * H + 2 * H * (W / 2 + 1); }

extern "C" int spv_spectrum_log1p(const float* img, void* out, int B, int C, int H, int W, int dtype, void* stream) {
    SPV_CHECK(B > 0 && C > 0 && H > 0 && W > 0, "spv_spectrum_log1p: empty problem B=%d C=%d H=%d W=%d", B, C, H, W);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_spectrum_log1p: bad dtype %d", dtype);
    const size_t lds = (size_t)spv_spectrum_floats(H, W) * sizeof(float);
    SPV_CHECK(lds <= 64 * 1024, "spv_spectrum_log1p: a %dx%d plane needs %zu bytes of LDS (limit 65536)", H, W, lds);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == SPV_F32)
        hipLaunchKernelGGL(spectrum_kernel<float>, dim3(B * C), dim3(256), lds, st, img, (float*)out, C, H, W);
    else
        hipLaunchKernelGGL(spectrum_kernel<bf16_t>, dim3(B * C), dim3(256), lds, st, img, (bf16_t*)out, C, H, W);
    SPV_LAUNCH_CHECK("spv_spectrum_log1p");
    SPV_COUNT_PATH(SPV_PATH_SPECTRUM);
    return 0;
}

extern "C" int spv_conv3x3_fwd(const void* x, const void* w, const float* bias, void* y, void* cols, int B, int H, int W, int Cin,
                               int Cout, int dtype, void* stream) {
    SPV_CHECK(B > 0 && H >= 3 && W >= 3 && Cin > 0 && Cout > 0, "spv_conv3x3_fwd: bad shape B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W,
              Cin, Cout);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_conv3x3_fwd: bad dtype %d", dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t M = (int64_t)B * (H - 2) * (W - 2);
    SPV_CHECK(M < (1LL << 31), "spv_conv3x3_fwd: %lld positions", (long long)M);
    const int Kp = round8(9 * Cin);
    const int64_t total = M * Kp;
    if (dtype == SPV_F32)
        hipLaunchKernelGGL((im2col_kernel<float, false>), dim3(grid_for(total)), dim3(256), 0, st, (const float*)x, (float*)cols, H, W, Cin,
                           M, (int64_t)Kp, total);
    else
        hipLaunchKernelGGL((im2col_kernel<bf16_t, false>), dim3(grid_for(total)), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)cols, H, W,
                           Cin, M, (int64_t)Kp, total);
    SPV_LAUNCH_CHECK("spv_conv3x3_fwd (gather)");
    const int rc = spv_gemm_nt(cols, w, bias, y, (int)M, Cout, Kp, Kp, Kp, Cout, dtype, dtype, 0, 1, nullptr, stream);
    if (rc) return rc;
    SPV_COUNT_PATH(SPV_PATH_CONV_FWD);
    return 0;
}

extern "C" int spv_conv3x3_dgrad(const void* dy, const void* wd, void* dx, void* cols, int B, int H, int W, int Cin, int Cout, int dtype,
                                 void* stream) {
    SPV_CHECK(B > 0 && H >= 3 && W >= 3 && Cin > 0 && Cout > 0, "spv_conv3x3_dgrad: bad shape B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W,
              Cin, Cout);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_conv3x3_dgrad: bad dtype %d", dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t M = (int64_t)B * H * W;
    SPV_CHECK(M < (1LL << 31), "spv_conv3x3_dgrad: %lld positions", (long long)M);
    const int Kd = round8(9 * Cout);
    const int64_t total = M * Kd;
    if (dtype == SPV_F32)
        hipLaunchKernelGGL(dcols_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, (const float*)dy, (float*)cols, H, W, Cout, Kd,
                           total);
    else
        hipLaunchKernelGGL(dcols_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, (const bf16_t*)dy, (bf16_t*)cols, H, W, Cout, Kd,
                           total);
    SPV_LAUNCH_CHECK("spv_conv3x3_dgrad (gather)");
    const int rc = spv_gemm_nt(cols, wd, nullptr, dx, (int)M, Cin, Kd, Kd, Kd, Cin, dtype, dtype, 0, 1, nullptr, stream);
    if (rc) return rc;
    SPV_COUNT_PATH(SPV_PATH_CONV_DGRAD);
    return 0;
}

extern "C" int spv_conv3x3_wgrad(const void* dy, const void* x, float* dw, void* dyt, void* colst, float* workspace, int splits, int B,
                                 int H, int W, int Cin, int Cout, int dtype, void* stream) {
    SPV_CHECK(B > 0 && H >= 3 && W >= 3 && Cin > 0 && Cout > 0, "spv_conv3x3_wgrad: bad shape B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W,
              Cin, Cout);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_conv3x3_wgrad: bad dtype %d", dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t M = (int64_t)B * (H - 2) * (W - 2);
    SPV_CHECK(M < (1LL << 31) - 8, "spv_conv3x3_wgrad: %lld positions", (long long)M);
    const int Mp = round8((int)M);
    const int K = 9 * Cin;
    const int64_t t1 = (int64_t)Cout * Mp, t2 = (int64_t)K * Mp;
    if (dtype == SPV_F32) {
        hipLaunchKernelGGL(transpose_rows_kernel<float>, dim3(grid_for(t1)), dim3(256), 0, st, (const float*)dy, (float*)dyt, M, Cout,
                           (int64_t)Mp, t1);
        hipLaunchKernelGGL((im2col_kernel<float, true>), dim3(grid_for(t2)), dim3(256), 0, st, (const float*)x, (float*)colst, H, W, Cin,
                           M, (int64_t)Mp, t2);
    } else {
        hipLaunchKernelGGL(transpose_rows_kernel<bf16_t>, dim3(grid_for(t1)), dim3(256), 0, st, (const bf16_t*)dy, (bf16_t*)dyt, M, Cout,
                           (int64_t)Mp, t1);
        hipLaunchKernelGGL((im2col_kernel<bf16_t, true>), dim3(grid_for(t2)), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)colst, H, W,
                           Cin, M, (int64_t)Mp, t2);
    }
    SPV_LAUNCH_CHECK("spv_conv3x3_wgrad (gather)");
    const int rc = spv_gemm_nt(dyt, colst, nullptr, dw, Cout, K, Mp, Mp, Mp, K, dtype, SPV_F32, 0, splits, workspace, stream);
    if (rc) return rc;
    SPV_COUNT_PATH(SPV_PATH_CONV_WGRAD);
    return 0;
}

extern "C" int spv_token_pool_fwd(const void* y, void* out, int B, int L, int C, int T, int ldo, int dtype, void* stream) {
    SPV_CHECK(B > 0 && L > 0 && C > 0 && T > 0 && ldo >= C, "spv_token_pool_fwd: bad shape B=%d L=%d C=%d T=%d ldo=%d", B, L, C, T, ldo);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_token_pool_fwd: bad dtype %d", dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t total = (int64_t)B * T * ldo;
    if (dtype == SPV_F32)
        hipLaunchKernelGGL(pool_fwd_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, (const float*)y, (float*)out, L, C, T, ldo, total);
    else
        hipLaunchKernelGGL(pool_fwd_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, (const bf16_t*)y, (bf16_t*)out, L, C, T, ldo,
                           total);
    SPV_LAUNCH_CHECK("spv_token_pool_fwd");
    SPV_COUNT_PATH(SPV_PATH_TOKEN_POOL);
    return 0;
}

extern "C" int spv_token_pool_bwd(const void* dout, int ldo, const void* add, void* dy, int B, int L, int C, int T, int dtype, void* stream) {
    SPV_CHECK(B > 0 && L > 0 && C > 0 && T > 0 && ldo >= C, "spv_token_pool_bwd: bad shape B=%d L=%d C=%d T=%d ldo=%d", B, L, C, T, ldo);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_token_pool_bwd: bad dtype %d", dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t total = (int64_t)B * L * C;
    if (dtype == SPV_F32)
        hipLaunchKernelGGL(pool_bwd_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, (const float*)dout, ldo, (const float*)add,
                           (float*)dy, L, C, T, total);
    else
        hipLaunchKernelGGL(pool_bwd_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, st, (const bf16_t*)dout, ldo, (const bf16_t*)add,
                           (bf16_t*)dy, L, C, T, total);
    SPV_LAUNCH_CHECK("spv_token_pool_bwd");
    SPV_COUNT_PATH(SPV_PATH_TOKEN_UNPOOL);
    return 0;
}
