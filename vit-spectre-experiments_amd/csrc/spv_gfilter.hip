// The learnable global-filter token mixer (include/spv.h):
//   X = rfft(x, tokens, ortho);  y = irfft(X * W, n = tokens, ortho)          W (K, dim) complex, K = tokens / 2 + 1
// as two real DFT products along the token axis with the pointwise complex multiply between them.  Every embedding column is
// independent, so a workgroup owns (sample, column block): a lane is a column, the four waves share the bins (then the tokens) four
// at a time, and the spectrum never leaves LDS.  Everything is fp32 in registers and LDS; the table is fp32 (cos, sin)(2 pi j /
// tokens), copied into LDS once per workgroup and read there at a wave-uniform index (a broadcast).  irfft ignores the imaginary
// part of the DC bin (and of the Nyquist bin of an even length): the kernels read those filter entries as 0 and write their gradient
// as a literal +0.
#include "spv_common.h"
#include "spv_gfilter_core.h"

constexpr int GFT = 256, GFW = GFT / 64;   // threads and waves of a workgroup

__global__ void gfilter_table_kernel(float* __restrict__ tab, int N) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    double s, c;
    sincospi(2.0 * (double)j / (double)N, &s, &c);
    tab[2 * j] = (float)c;
    tab[2 * j + 1] = (float)s;
}

// GKT bins (or tokens) per thread and pass: one LDS read of the data feeds 2 GKT multiply-adds.  The table entries, whose index is the
// same in every lane, are LDS broadcasts: read from global memory at a uniform address they become scalar loads, each waited for on its
// own, and that chain of latencies was the whole run time.  Each sum still runs over n (or k) in ascending order.
constexpr int GKT = 4;

// bins kk[0..GKT) of NV columns held in LDS as v[i][n * cb]: c[i][j] = sum_n cos(2 pi kk[j] n / N) v[i][n], s[i][j] likewise with sin
template <int NV>
__device__ __forceinline__ void gfilter_bins(const float* const (&v)[NV], const float* __restrict__ tab, int N, int cb, const int (&kk)[GKT],
                                             float (&c)[NV][GKT], float (&s)[NV][GKT]) {
    int m[GKT];
#pragma unroll
    for (int j = 0; j < GKT; ++j) {
        m[j] = 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) c[i][j] = s[i][j] = 0.0f;
    }
#pragma unroll 2
    for (int n = 0; n < N; ++n) {
        float e[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) e[i] = v[i][n * cb];
#pragma unroll
        for (int j = 0; j < GKT; ++j) {
            const float tc = tab[2 * m[j]], ts = tab[2 * m[j] + 1];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                c[i][j] = fmaf(tc, e[i], c[i][j]);
                s[i][j] = fmaf(ts, e[i], s[i][j]);
            }
            m[j] += kk[j];
            if (m[j] >= N) m[j] -= N;
        }
    }
}

// tokens nn[0..GKT) of one column from its weighted spectrum zr / zi [k * cb]: a[j] = sum_k zr[k] cos(2 pi k nn[j] / N) - zi[k] sin(..)
__device__ __forceinline__ void gfilter_tokens(const float* __restrict__ zr, const float* __restrict__ zi, const float* __restrict__ tab, int N,
                                               int K, int cb, const int (&nn)[GKT], float (&a)[GKT]) {
    int m[GKT];
#pragma unroll
    for (int j = 0; j < GKT; ++j) {
        m[j] = 0;
        a[j] = 0.0f;
    }
#pragma unroll 2
    for (int k = 0; k < K; ++k) {
        const float r = zr[k * cb], i = -zi[k * cb];
#pragma unroll
        for (int j = 0; j < GKT; ++j) {
            a[j] = fmaf(r, tab[2 * m[j]], a[j]);
            a[j] = fmaf(i, tab[2 * m[j] + 1], a[j]);
            m[j] += nn[j];
            if (m[j] >= N) m[j] -= N;
        }
    }
}

// y[n][lane] for the tokens of this wave, GKT at a time (the last group repeats token N - 1 and stores it once)
template <typename T>
__device__ __forceinline__ void gfilter_store_tokens(T* __restrict__ y, const float* __restrict__ zr, const float* __restrict__ zi,
                                                     const float* __restrict__ tab, int N, int K, int D, int cb, int wave) {
    for (int n0 = wave * GKT; n0 < N; n0 += GFW * GKT) {
        int nn[GKT];
        float a[GKT];
#pragma unroll
        for (int j = 0; j < GKT; ++j) nn[j] = min(n0 + j, N - 1);
        gfilter_tokens(zr, zi, tab, N, K, cb, nn, a);
#pragma unroll
        for (int j = 0; j < GKT; ++j)
            if (n0 + j < N) io<T>::st(y + (size_t)(n0 + j) * D, a[j]);
    }
}

// grid: batch * blocks, blocks = cdiv(D, cb).  LDS: xs [N][cb], zr / zi [K][cb], ts [N][2].
template <typename T>
__global__ __launch_bounds__(GFT) void gfilter_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ y,
                                                          const float* __restrict__ tab, int N, int D, int cb, int blocks, float inv_n) {
    extern __shared__ float lds[];
    const int K = N / 2 + 1;
    float* xs = lds;
    float* zr = xs + N * cb;
    float* zi = zr + K * cb;
    float* ts = zi + K * cb;   // the table, [N][2]
    const int b = blockIdx.x / blocks, c0 = (blockIdx.x % blocks) * cb;
    const int nc = min(cb, D - c0);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool on = lane < nc;
    const size_t base = (size_t)b * N * D + c0 + lane;
    for (int i = threadIdx.x; i < 2 * N; i += GFT) ts[i] = tab[i];
    if (on)
        for (int n = wave; n < N; n += GFW) xs[n * cb + lane] = io<T>::ld(x + base + (size_t)n * D);
    __syncthreads();
    if (on)
        for (int k0 = wave * GKT; k0 < K; k0 += GFW * GKT) {
            int kk[GKT];
#pragma unroll
            for (int j = 0; j < GKT; ++j) kk[j] = min(k0 + j, K - 1);
            const float* const v[1] = {xs + lane};
            float c[1][GKT], s[1][GKT];
            gfilter_bins<1>(v, ts, N, cb, kk, c, s);            // X = c - i s (un-normalised)
#pragma unroll
            for (int j = 0; j < GKT; ++j) {
                const int k = k0 + j;
                if (k >= K) break;
                const bool inert = k == 0 || 2 * k == N;
                const float* wp = w + ((size_t)k * D + c0 + lane) * 2;
                const float wr = wp[0], wi = inert ? 0.0f : wp[1];
                const float ck = (inert ? 1.0f : 2.0f) * inv_n;
                zr[k * cb + lane] = ck * fmaf(c[0][j], wr, s[0][j] * wi);    // Re((c - i s)(wr + i wi))
                zi[k * cb + lane] = ck * fmaf(c[0][j], wi, -s[0][j] * wr);   // Im
            }
        }
    __syncthreads();
    if (on) gfilter_store_tokens<T>(y + base, zr + lane, zi + lane, ts, N, K, D, cb, wave);
}

// grid: slabs * blocks.  Workgroup (slab g, column block) owns samples g, g + slabs, ...; every (bin, column) of its slab belongs to
// one thread from the first sample to the last, so the sum over its samples has one order and needs no atomic.
// LDS: xs / gs [N][cb], zr / zi / ar / ai [K][cb], ts [N][2].
template <typename T>
__global__ __launch_bounds__(GFT) void gfilter_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ w,
                                                          T* __restrict__ dx, float* __restrict__ partials, const float* __restrict__ tab,
                                                          int B, int N, int D, int cb, int blocks, int slabs, float inv_n) {
    extern __shared__ float lds[];
    const int K = N / 2 + 1;
    float* xs = lds;
    float* gs = xs + N * cb;
    float* zr = gs + N * cb;
    float* zi = zr + K * cb;
    float* ar = zi + K * cb;
    float* ai = ar + K * cb;
    float* ts = ai + K * cb;   // the table, [N][2]
    const int g = blockIdx.x / blocks, c0 = (blockIdx.x % blocks) * cb;
    const int nc = min(cb, D - c0);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool on = lane < nc;
    for (int i = threadIdx.x; i < 2 * N; i += GFT) ts[i] = tab[i];
    if (on)
        for (int k = wave; k < K; k += GFW) {
            ar[k * cb + lane] = 0.0f;
            ai[k * cb + lane] = 0.0f;
        }
    for (int b = g; b < B; b += slabs) {
        const size_t base = (size_t)b * N * D + c0 + lane;
        __syncthreads();   // the previous sample's dx pass has read zr / zi
        if (on)
            for (int n = wave; n < N; n += GFW) {
                xs[n * cb + lane] = io<T>::ld(x + base + (size_t)n * D);
                gs[n * cb + lane] = io<T>::ld(dy + base + (size_t)n * D);
            }
        __syncthreads();
        if (on)
            for (int k0 = wave * GKT; k0 < K; k0 += GFW * GKT) {
                int kk[GKT];
#pragma unroll
                for (int j = 0; j < GKT; ++j) kk[j] = min(k0 + j, K - 1);
                const float* const v[2] = {xs + lane, gs + lane};
                float c[2][GKT], s[2][GKT];                         // X = c[0] - i s[0], G = c[1] - i s[1] (un-normalised)
                gfilter_bins<2>(v, ts, N, cb, kk, c, s);
#pragma unroll
                for (int j = 0; j < GKT; ++j) {
                    const int k = k0 + j;
                    if (k >= K) break;
                    const float cx = c[0][j], sx = s[0][j], cg = c[1][j], sg = s[1][j];
                    const bool inert = k == 0 || 2 * k == N;
                    const float* wp = w + ((size_t)k * D + c0 + lane) * 2;
                    const float wr = wp[0], wi = inert ? 0.0f : wp[1];
                    const float ck = (inert ? 1.0f : 2.0f) * inv_n;
                    zr[k * cb + lane] = ck * fmaf(cg, wr, -sg * wi);    // Re((cg - i sg)(wr - i wi))
                    zi[k * cb + lane] = -ck * fmaf(sg, wr, cg * wi);    // Im
                    ar[k * cb + lane] += ck * fmaf(cx, cg, sx * sg);    // Re(conj(X) G)
                    ai[k * cb + lane] += ck * fmaf(sx, cg, -cx * sg);   // Im
                }
            }
        __syncthreads();
        if (on) gfilter_store_tokens<T>(dx + base, zr + lane, zi + lane, ts, N, K, D, cb, wave);
    }
    if (on)
        for (int k = wave; k < K; k += GFW) {
            const bool inert = k == 0 || 2 * k == N;
            float* o = partials + (((size_t)g * K + k) * D + c0 + lane) * 2;
            o[0] = ar[k * cb + lane];
            o[1] = inert ? 0.0f : ai[k * cb + lane];
        }
}

// ---------------------------------------------------------------- the fast path (bf16, dim % 64 == 0, tokens <= 80, 16-byte aligned)
// Both token-axis products on v_mfma_f32_32x32x16_bf16.  A workgroup owns (sample, 64 columns); x is read once with 16-byte loads and
// kept in LDS transposed ([column][token], bf16 -- exact), so that a B fragment (8 consecutive k of one column) is one 16-byte read.
//   1. [C; S] = [Fc; Fs] . x      Fc / Fs (bins x tokens) as hi + lo bf16 tables, two MFMAs per step: the table is exact to 2^-17.
//      Wave w owns the bin tile w / 2 and the column tile w % 2, and holds C and S of the same (bin, column) in the same register.
//   2. Z = c_k / N . X W_eff in fp32 registers, written to LDS transposed as hi + lo bf16 (the sine part negated).
//   3. y = Gc . Zr + Gs . (-Zi)   Gc / Gs (tokens x bins) hi + lo: hi.hi + lo.hi + hi.lo, three MFMAs per term and step.
// The backward does step 1 for x and dy at once, keeps c_k / N . conj(X) G in registers over the samples it owns, and writes one slab.
// A fragments come straight from the tables in global memory (90 KiB at most, shared by every workgroup).
// Fragment order (as in spv_hadamard.hip): lane l holds A[row = l & 31][k = 8 (l >> 5) + e], B[k = 8 (l >> 5) + e][col = l & 31] and
// C[row = (r & 3) + 8 (r >> 2) + 4 (l >> 5)][col = l & 31].
constexpr int GFX_NPS = GFILTER_FAST_MAX_TOKENS + 8;   // LDS row stride of a transposed operand, in bf16: 16-byte rows, odd in 16-byte units
constexpr int GFX_KPS = 64 + 8;                         // ... of the transposed spectrum

__global__ void gfilter_fast_table_kernel(bf16_t* __restrict__ tab, int N) {
    const int K = N / 2 + 1, NP = gfilter_fast_np(N), NPO = gfilter_fast_npo(N), KP = gfilter_fast_kp(N);
    const int t1 = 4 * KP * NP, total = t1 + 4 * NPO * KP;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    int h, part, k, n;
    if (e < t1) {
        h = e / (2 * KP * NP);
        int r = e % (2 * KP * NP);
        part = r / (KP * NP);
        r %= KP * NP;
        k = r / NP;
        n = r % NP;
    } else {
        const int q = e - t1;
        h = q / (2 * NPO * KP);
        int r = q % (2 * NPO * KP);
        part = r / (NPO * KP);
        r %= NPO * KP;
        n = r / KP;
        k = r % KP;
    }
    float v = 0.0f;
    if (k < K && n < N) {
        double sn, cs;
        sincospi(2.0 * (double)((k * n) % N) / (double)N, &sn, &cs);
        v = part ? (float)sn : (float)cs;
    }
    const bf16_t hi = f2bf(v);
    tab[e] = h ? f2bf(v - bf2f(hi)) : hi;
}

template <int BWD>
__global__ __launch_bounds__(GFT) void gfilter_fast_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, const float* __restrict__ w,
                                                           bf16_t* __restrict__ out, float* __restrict__ partials,
                                                           const bf16_t* __restrict__ tab, int B, int N, int D, int slabs, float inv_n) {
    __shared__ __attribute__((aligned(16))) bf16_t xT[(1 + BWD) * 64 * GFX_NPS];
    __shared__ __attribute__((aligned(16))) bf16_t zT[4 * 64 * GFX_KPS];
    const int K = N / 2 + 1, NP = gfilter_fast_np(N), NPO = gfilter_fast_npo(N), KP = gfilter_fast_kp(N);
    const bf16_t* T1 = tab;
    const bf16_t* T2 = tab + 4 * KP * NP;
    const int blocks = D / 64;
    const int g0 = blockIdx.x / blocks, c0 = (blockIdx.x % blocks) * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, g = lane >> 5;
    const int rt = wave >> 1, ct = wave & 1;
    const bool pair = rt * 32 < KP;   // this wave has a (bin tile, column tile) of step 1
    f32x16 ar, ai;
#pragma unroll
    for (int r = 0; r < 16; ++r) ar[r] = ai[r] = 0.0f;
    for (int b = g0; b < B; b += (BWD ? slabs : B)) {
        const size_t base = (size_t)b * N * D + c0;
        // ---- x (and dy) into LDS, transposed; tokens N .. NP - 1 are zeros
        for (int idx = tid; idx < NP * 8; idx += GFT) {
            const int n = idx >> 3, seg = idx & 7;
#pragma unroll
            for (int v = 0; v <= BWD; ++v) {
                uint4 q = make_uint4(0u, 0u, 0u, 0u);
                if (n < N) q = *reinterpret_cast<const uint4*>((v ? dy : x) + base + (size_t)n * D + seg * 8);
                const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    xT[(v * 64 + seg * 8 + e) * GFX_NPS + n] = (bf16_t)((e & 1) ? (u[e >> 1] >> 16) : (u[e >> 1] & 0xffffu));
            }
        }
        __syncthreads();
        // ---- 1. the spectra, 2. the filter
        if (pair) {
            f32x16 aC[1 + BWD], aS[1 + BWD];
#pragma unroll
            for (int v = 0; v <= BWD; ++v)
#pragma unroll
                for (int r = 0; r < 16; ++r) aC[v][r] = aS[v][r] = 0.0f;
            for (int ks = 0; ks < NP / 16; ++ks) {
                const int k0 = ks * 16 + 8 * g;
                bf16x8 bfr[1 + BWD];
#pragma unroll
                for (int v = 0; v <= BWD; ++v) bfr[v] = *reinterpret_cast<const bf16x8*>(&xT[(v * 64 + ct * 32 + c) * GFX_NPS + k0]);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bf16x8 fc = *reinterpret_cast<const bf16x8*>(T1 + ((size_t)(h * 2 + 0) * KP + rt * 32 + c) * NP + k0);
                    const bf16x8 fs = *reinterpret_cast<const bf16x8*>(T1 + ((size_t)(h * 2 + 1) * KP + rt * 32 + c) * NP + k0);
#pragma unroll
                    for (int v = 0; v <= BWD; ++v) {
                        aC[v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fc, bfr[v], aC[v], 0, 0, 0);
                        aS[v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fs, bfr[v], aS[v], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g, col = ct * 32 + c;
                float zr = 0.0f, zi = 0.0f;
                if (k < K) {
                    const bool inert = k == 0 || 2 * k == N;
                    const float* wp = w + ((size_t)k * D + c0 + col) * 2;
                    const float wr = wp[0], wi = inert ? 0.0f : wp[1];
                    const float ck = (inert ? 1.0f : 2.0f) * inv_n;
                    if constexpr (!BWD) {
                        const float cc = aC[0][r], ss = aS[0][r];            // X = cc - i ss (un-normalised)
                        zr = ck * fmaf(cc, wr, ss * wi);                     // Re(X W)
                        zi = ck * fmaf(cc, wi, -ss * wr);                    // Im
                    } else {
                        const float cx = aC[0][r], sx = aS[0][r], cg = aC[BWD][r], sg = aS[BWD][r];
                        zr = ck * fmaf(cg, wr, -sg * wi);                    // Re(G conj(W))
                        zi = -ck * fmaf(sg, wr, cg * wi);                    // Im
                        ar[r] += ck * fmaf(cx, cg, sx * sg);                 // Re(conj(X) G)
                        ai[r] += ck * fmaf(sx, cg, -cx * sg);                // Im
                    }
                }
                zi = -zi;   // step 3 adds Gs . (-Zi)
                const bf16_t zrh = f2bf(zr), zih = f2bf(zi);
                bf16_t* z = &zT[col * GFX_KPS + k];
                z[0] = zrh;
                z[64 * GFX_KPS] = f2bf(zr - bf2f(zrh));
                z[2 * 64 * GFX_KPS] = zih;
                z[3 * 64 * GFX_KPS] = f2bf(zi - bf2f(zih));
            }
        }
        __syncthreads();
        // ---- 3. back to tokens
        for (int t = wave; t < (NPO / 32) * 2; t += GFW) {
            const int mt = t >> 1, ct3 = t & 1;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            for (int ks = 0; ks < KP / 16; ++ks) {
                const int k0 = ks * 16 + 8 * g;
                const bf16_t* z = &zT[(ct3 * 32 + c) * GFX_KPS + k0];
                const bf16x8 zrh = *reinterpret_cast<const bf16x8*>(z), zrl = *reinterpret_cast<const bf16x8*>(z + 64 * GFX_KPS);
                const bf16x8 zih = *reinterpret_cast<const bf16x8*>(z + 2 * 64 * GFX_KPS), zil = *reinterpret_cast<const bf16x8*>(z + 3 * 64 * GFX_KPS);
                const bf16_t* t2 = T2 + ((size_t)mt * 32 + c) * KP + k0;
                const size_t plane = (size_t)NPO * KP;   // [hi, lo][cos, sin] planes
                const bf16x8 gch = *reinterpret_cast<const bf16x8*>(t2), gsh = *reinterpret_cast<const bf16x8*>(t2 + plane);
                const bf16x8 gcl = *reinterpret_cast<const bf16x8*>(t2 + 2 * plane), gsl = *reinterpret_cast<const bf16x8*>(t2 + 3 * plane);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gch, zrh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gsh, zih, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gcl, zrh, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gsl, zih, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gch, zrl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gsh, zil, acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
                if (n < N) out[base + (size_t)n * D + ct3 * 32 + c] = f2bf(acc[r]);
            }
        }
    }
    if constexpr (BWD) {
        if (pair) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g;
                if (k < K) {
                    const bool inert = k == 0 || 2 * k == N;
                    float* o = partials + (((size_t)g0 * K + k) * D + c0 + ct * 32 + c) * 2;
                    o[0] = ar[r];
                    o[1] = inert ? 0.0f : ai[r];
                }
            }
        }
    }
}

static bool gfilter_aligned16(const void* a, const void* b, const void* c, const void* d) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15u) == 0;
}

__global__ __launch_bounds__(FOLD_COLS* FOLD_ROWS) void gfilter_fold_kernel(FoldJob j) { fold_partials_block<1>(j, blockIdx.x, threadIdx.x); }

static const char* gfilter_refusal(int path) {
    switch (path) {
        case GFILTER_REFUSE_EMPTY: return "empty shape";
        case GFILTER_REFUSE_DTYPE: return "unknown dtype";
        case GFILTER_REFUSE_TOKENS: return "too many tokens for one column in LDS";
        case GFILTER_REFUSE_ALIGN: return "x, y (dy, dx) and tables must be 16-byte aligned on the fast path";
        default: return "refused";
    }
}

extern "C" int spv_gfilter_path(int dtype, int tokens, int dim, int aligned) { return gfilter_select(dtype, tokens, dim, aligned != 0).path; }
extern "C" int64_t spv_gfilter_table_floats(int tokens) { return gfilter_table_floats(tokens); }
extern "C" int64_t spv_gfilter_workspace_floats(int batch, int tokens, int dim) { return gfilter_workspace_floats(batch, tokens, dim); }
extern "C" int64_t spv_gfilter_partial_floats(int batch, int tokens, int dim) { return gfilter_partial_floats(batch, tokens, dim); }

extern "C" int spv_gfilter_make_tables(float* tables, int tokens, void* stream) {
    SPV_CHECK(tokens >= 1, "spv_gfilter_make_tables: empty shape (tokens=%d)", tokens);
    SPV_CHECK(tables, "spv_gfilter_make_tables: null pointer");
    hipLaunchKernelGGL(gfilter_table_kernel, dim3(cdiv(tokens, 256)), dim3(256), 0, (hipStream_t)stream, tables, tokens);
    SPV_LAUNCH_CHECK("spv_gfilter_make_tables");
    if (tokens <= GFILTER_FAST_MAX_TOKENS) {
        const int64_t n = gfilter_fast_t1(tokens) + gfilter_fast_t2(tokens);
        hipLaunchKernelGGL(gfilter_fast_table_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<bf16_t*>(tables + gfilter_generic_table_floats(tokens)), tokens);
        SPV_LAUNCH_CHECK("spv_gfilter_make_tables(fast)");
    }
    return 0;
}

extern "C" int spv_gfilter_fwd(const void* x, const float* filter, void* y, const float* tables, int batch, int tokens, int dim, int dtype,
                               float* workspace, void* stream) {
    (void)workspace;
    const GfilterPlan p = gfilter_select(dtype, tokens, dim, gfilter_aligned16(x, y, tables, nullptr));
    SPV_CHECK(batch >= 1 || p.path < 0, "spv_gfilter_fwd: empty shape (batch=%d)", batch);
    SPV_CHECK(p.path > 0, "spv_gfilter_fwd: %s (tokens=%d dim=%d dtype=%d)", gfilter_refusal(p.path), tokens, dim, dtype);
    SPV_CHECK(x && filter && y && tables, "spv_gfilter_fwd: null pointer");
    const int cb = p.cols_fwd, blocks = cdiv(dim, cb);
    SPV_CHECK((int64_t)batch * blocks <= 0x7fffffff, "spv_gfilter_fwd: too many workgroups");
    const size_t lds = ((size_t)cb * (tokens + 2 * p.bins) + 2 * (size_t)tokens) * sizeof(float);
    const float inv_n = (float)(1.0 / (double)tokens);
    hipStream_t st = (hipStream_t)stream;
    if (p.path == GFILTER_FAST) {
        hipLaunchKernelGGL(gfilter_fast_kernel<0>, dim3(batch * blocks), dim3(GFT), 0, st, (const bf16_t*)x, (const bf16_t*)nullptr, filter,
                           (bf16_t*)y, (float*)nullptr, reinterpret_cast<const bf16_t*>(tables + gfilter_generic_table_floats(tokens)), batch,
                           tokens, dim, 0, inv_n);
        SPV_LAUNCH_CHECK("spv_gfilter_fwd(fast)");
        return 0;
    }
    if (dtype == SPV_BF16)
        hipLaunchKernelGGL(gfilter_fwd_kernel<bf16_t>, dim3(batch * blocks), dim3(GFT), lds, st, (const bf16_t*)x, filter, (bf16_t*)y, tables, tokens,
                           dim, cb, blocks, inv_n);
    else
        hipLaunchKernelGGL(gfilter_fwd_kernel<float>, dim3(batch * blocks), dim3(GFT), lds, st, (const float*)x, filter, (float*)y, tables, tokens,
                           dim, cb, blocks, inv_n);
    SPV_LAUNCH_CHECK("spv_gfilter_fwd");
    return 0;
}

extern "C" int spv_gfilter_bwd(const void* x, const void* dy, const float* filter, void* dx, float* dfilter, const float* tables,
                               float* partials, int batch, int tokens, int dim, int dtype, float* workspace, void* stream) {
    (void)workspace;
    const GfilterPlan p = gfilter_select(dtype, tokens, dim, gfilter_aligned16(x, dy, dx, tables));
    SPV_CHECK(batch >= 1 || p.path < 0, "spv_gfilter_bwd: empty shape (batch=%d)", batch);
    SPV_CHECK(p.path > 0, "spv_gfilter_bwd: %s (tokens=%d dim=%d dtype=%d)", gfilter_refusal(p.path), tokens, dim, dtype);
    SPV_CHECK(x && dy && filter && dx && dfilter && tables && partials, "spv_gfilter_bwd: null pointer");
    const int cb = p.cols_bwd, blocks = cdiv(dim, cb), slabs = gfilter_slabs(batch);
    const int64_t total = (int64_t)p.bins * dim * 2;
    SPV_CHECK(total <= 0x7fffffff, "spv_gfilter_bwd: filter too large");
    const size_t lds = ((size_t)cb * (2 * tokens + 4 * p.bins) + 2 * (size_t)tokens) * sizeof(float);
    const float inv_n = (float)(1.0 / (double)tokens);
    hipStream_t st = (hipStream_t)stream;
    if (p.path == GFILTER_FAST)
        hipLaunchKernelGGL(gfilter_fast_kernel<1>, dim3(slabs * blocks), dim3(GFT), 0, st, (const bf16_t*)x, (const bf16_t*)dy, filter,
                           (bf16_t*)dx, partials, reinterpret_cast<const bf16_t*>(tables + gfilter_generic_table_floats(tokens)), batch, tokens,
                           dim, slabs, inv_n);
    else if (dtype == SPV_BF16)
        hipLaunchKernelGGL(gfilter_bwd_kernel<bf16_t>, dim3(slabs * blocks), dim3(GFT), lds, st, (const bf16_t*)x, (const bf16_t*)dy, filter,
                           (bf16_t*)dx, partials, tables, batch, tokens, dim, cb, blocks, slabs, inv_n);
    else
        hipLaunchKernelGGL(gfilter_bwd_kernel<float>, dim3(slabs * blocks), dim3(GFT), lds, st, (const float*)x, (const float*)dy, filter,
                           (float*)dx, partials, tables, batch, tokens, dim, cb, blocks, slabs, inv_n);
    SPV_LAUNCH_CHECK("spv_gfilter_bwd");
    FoldJob j = {};
    j.partials = partials;
    j.o[0] = dfilter;
    j.parts = slabs;
    j.np = 1;
    j.n = (int)total;
    hipLaunchKernelGGL(gfilter_fold_kernel, dim3(cdiv(total, FOLD_COLS)), dim3(FOLD_COLS * FOLD_ROWS), 0, st, j);
    SPV_LAUNCH_CHECK("spv_gfilter_bwd(fold)");
    return 0;
}
