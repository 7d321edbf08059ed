// spv_patch.hip -- patch-embedding plumbing around the MFMA GEMM: pixel-block extraction, CLS/position rows,
// the SpectralPatchEmbed weight fold (Re(rfft2 ortho) and the learnable frequency weights folded into the
// projection matrix), dropout as a stand-alone counter-based mask.
#define SPV_USES_SEED
#include "spv_common.h"
#include "spv_prologue_core.h"
#include "spv_token_embed_core.h"

#include <type_traits>

namespace {

__device__ __forceinline__ float ld_any(const void* base, size_t off, int bf) {
    return bf ? bf2f(static_cast<const bf16_t*>(base)[off]) : static_cast<const float*>(base)[off];
}

// the float-image patch rows: bodies in spv_prologue_core.h (shared with the step prologue)
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img, void* __restrict__ out, int B, int C, int H,
                                                       int W, int P, int ld, int transposed, int bf) {
    patchify_body(img, out, B, C, H, W, P, ld, transposed, bf, blockIdx.x, gridDim.x);
}

template <typename T>
__global__ __launch_bounds__(256) void patchify_vec4_kernel(const float* __restrict__ img, T* __restrict__ out, int B, int C, int H, int W,
                                                            int P, int ld, int token_rows) {
    patchify_vec4_body<T>(img, out, B, C, H, W, P, ld, token_rows, blockIdx.x, gridDim.x);
}

// The same patch rows straight from the loader's uint8 HWC image (spectre_vit/repl/train.py:102-112: ToTensor = /255,
// then Normalize(mean, std) per channel): out = (img[b][y][x][c] / 255 - mean[c]) * inv_std[c].  One pass instead of
// host-side float conversion + normalise + NCHW copy + patchify.
__global__ __launch_bounds__(256) void patchify_u8_kernel(const unsigned char* __restrict__ img, const float* __restrict__ mean,
                                                          const float* __restrict__ inv_std, void* __restrict__ out, int B, int C,
                                                          int H, int W, int P, int ld, int transposed, int bf) {
    const int nH = H / P, nW = W / P, Np = nH * nW, K = C * P * P;
    const int64_t rows = (int64_t)B * Np;
    // transposed == 2: token rows [B][Np + 1][ld], row 0 of every image (the CLS slot) zero -- the layout the token GEMM and the TN
    // weight-gradient GEMM both read as it lies
    const int64_t total = transposed == 1 ? (int64_t)K * ld : (transposed == 2 ? (int64_t)B * (Np + 1) * ld : rows * ld);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
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
            const float px = (float)img[(((size_t)b * H + ih * P + p) * W + iw * P + q) * C + c];
            v = (px * (1.0f / 255.0f) - mean[c]) * inv_std[c];
        }
        st_any(out, (size_t)e, bf, v);
    }
}

__global__ __launch_bounds__(256) void posbias_kernel(const float* __restrict__ pos, const float* __restrict__ bias,
                                                      const float* __restrict__ cls, float* __restrict__ out, int Np, int E) {
    posbias_body(pos, bias, cls, out, Np, E, blockIdx.x, gridDim.x);
}

// tokens[b][0][e] = cls[e] + pos[0][e]
__global__ __launch_bounds__(256) void cls_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                                       void* __restrict__ tokens, int B, int T, int E, int bf) {
    const int total = B * E;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int b = i / E, e = i % E;
        st_any(tokens, ((size_t)b * T) * E + e, bf, cls[e] + pos[e]);
    }
}

// mask(i) = hash(key(i >> 12), i & 4095): 8 consecutive elements per thread share the block key and four pair hashes
// (16-byte bf16 / 2 x 16-byte fp32 accesses); the scalar form spent three hashes on every element
__global__ __launch_bounds__(256) void dropout_kernel(const void* __restrict__ x, void* __restrict__ y, int64_t n, float p,
                                                      uint64_t seed, int bf) {
    const float inv_keep = 1.0f / (1.0f - p);
    const int64_t n8 = n >> 3;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n8; v += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = v << 3;
        const unsigned key = dropout_row_key(live_seed(seed), (uint64_t)i >> 12);
        const unsigned c0 = (unsigned)(i & 4095);
        float sc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) sc[u] = dropout_scale(key, c0 + u, p, inv_keep);
        if (bf) {
            const uint4 t = *reinterpret_cast<const uint4*>(static_cast<const bf16_t*>(x) + i);
            const unsigned w[4] = {t.x, t.y, t.z, t.w};
            unsigned o[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                o[u] = pack_bf16x2(__uint_as_float(w[u] << 16) * sc[2 * u], __uint_as_float(w[u] & 0xffff0000u) * sc[2 * u + 1]);
            *reinterpret_cast<uint4*>(static_cast<bf16_t*>(y) + i) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            const float4 a = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + i);
            const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(x) + i + 4);
            *reinterpret_cast<float4*>(static_cast<float*>(y) + i) = make_float4(a.x * sc[0], a.y * sc[1], a.z * sc[2], a.w * sc[3]);
            *reinterpret_cast<float4*>(static_cast<float*>(y) + i + 4) = make_float4(b.x * sc[4], b.y * sc[5], b.z * sc[6], b.w * sc[7]);
        }
    }
    // ragged tail (n not a multiple of 8): scalar
    for (int64_t i = (n8 << 3) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        st_any(y, (size_t)i, bf, ld_any(x, (size_t)i, bf) *
                                     dropout_scale(dropout_row_key(live_seed(seed), (uint64_t)i >> 12), (unsigned)(i & 4095), p, inv_keep));
}

__global__ __launch_bounds__(256) void spectral_fold_kernel(const float* __restrict__ w, const float* __restrict__ fh,
                                                            const float* __restrict__ fw, float* __restrict__ wf, int E, int C, int P,
                                                            bf16_t* __restrict__ wf_bf = nullptr) {
    spectral_fold_body(w, fh, fw, wf, E, C, P, wf_bf, blockIdx.x, gridDim.x);
}

// G[e][c,u,v] = sum_{p,q} dWf[e][c,p,q] R[(u,v),(p,q)];  dW = G fh fw;  gw = G * W (for the frequency-weight sums)
__global__ __launch_bounds__(256) void spectral_fold_bwd_kernel(const float* __restrict__ dwf, const float* __restrict__ w,
                                                                const float* __restrict__ fh, const float* __restrict__ fw,
                                                                float* __restrict__ dw, float* __restrict__ gw, int E, int C, int P) {
    const int Pv = P / 2 + 1;
    const int total = E * C * P * Pv;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int v = i % Pv, u = (i / Pv) % P, ec = i / (Pv * P);
        const float* dr = dwf + (size_t)ec * P * P;
        float g = 0.0f;
        for (int p = 0; p < P; ++p)
            for (int q = 0; q < P; ++q) g = fmaf(dr[p * P + q], rcoef(u, v, p, q, P), g);
        dw[i] = g * fh[u] * fw[v];
        gw[i] = g * w[i];
    }
}
// dfh[u] = sum_{e,c,v} gw fw[v];  dfw[v] = sum_{e,c,u} gw fh[u]; single workgroup (power-of-two size), fixed summation order: each
// thread's (e,c) slices into its own LDS row, then a binary tree over the rows.  (256 threads and a serial 256-term tail: 14.5 us for
// 18 432 numbers; this form ~4 us.)
__global__ __launch_bounds__(1024) void freq_weight_grad_kernel(const float* __restrict__ gw, const float* __restrict__ fh,
                                                                const float* __restrict__ fw, float* __restrict__ dfh,
                                                                float* __restrict__ dfw, int EC, int P) {
    extern __shared__ float lds[];  // [blockDim.x][P + Pv]
    const int Pv = P / 2 + 1, S = P + Pv;
    const int nt = blockDim.x;
    float* mine = lds + threadIdx.x * S;
    for (int j = 0; j < S; ++j) mine[j] = 0.0f;
    for (int ec = threadIdx.x; ec < EC; ec += nt) {
        const float* g = gw + (size_t)ec * P * Pv;
        for (int u = 0; u < P; ++u)
            for (int v = 0; v < Pv; ++v) {
                const float t = g[u * Pv + v];
                mine[u] += t * fw[v];
                mine[P + v] += t * fh[u];
            }
    }
    for (int stride = nt >> 1; stride >= 1; stride >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < stride) {
            const float* other = lds + (threadIdx.x + stride) * S;
            for (int j = 0; j < S; ++j) mine[j] += other[j];
        }
    }
    if (threadIdx.x == 0) {
        for (int j = 0; j < P; ++j) dfh[j] = mine[j];
        for (int j = 0; j < Pv; ++j) dfw[j] = mine[P + j];
    }
}

inline int ew_blocks(int64_t n) { return patch_ew_blocks(n); }

// ---- the token GEMM of the embedding's forward: tokens[r] = bf16((patches[r] . w^T + posbias[r % T]) * dropout_scale), K = 16 KS <= 64.
// The launch is 34 MB of output behind 1.6 GFLOP: on the 128 x 128 tile kernel each of its 1040 single-K-step tiles paid two operand
// stagings and four workgroup barriers.  Here a WAVE is the unit (plan: spv_token_embed_core.h): it loads its 64-column share of w once,
// as the B fragments of v_mfma_f32_32x32x16_bf16 (2 x KS uint4), and walks 32-row blocks.  Both operands are K-contiguous, so the A
// fragment of a lane is 16 contiguous bytes of one patch row: a plain 16-byte load, no LDS staging.  The accumulators leave through a
// wave-private fp32 stage, 16 rows at a time, so that a lane holds 8 consecutive columns of one row: each store instruction of the wave
// writes 8 whole 128-byte lines.  No workgroup barrier: a wave's LDS accesses run in order.  The next block's loads go out before this
// block's stores (see the loop).
// Operand roles, k order and the epilogue (+ posbias row, * dropout scale, one pack per pair) are those of gemm_nt_kernel +
// store_acc_tile, whose K padding adds exact zeros: the output is that call's bit for bit.
template <int KS>
__global__ __launch_bounds__(64 * TE_WAVES, 3) void token_embed_kernel(const bf16_t* __restrict__ P, const bf16_t* __restrict__ Wt,
                                                                    const float* __restrict__ posbias, bf16_t* __restrict__ out, int rows,
                                                                    int n, int T, int shares, int walkers, float p, uint64_t seed) {
    constexpr int K = 16 * KS;
    constexpr int SLD = TE_COLS + 4;   // fp32 words per stage row (rows 16 bytes apart in the banks, as in store_acc_tile)
    __shared__ __attribute__((aligned(16))) float stage_all[TE_WAVES][16 * SLD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * TE_WAVES + wave;
    if (g >= shares * walkers) return;   // (the last workgroup's spare waves; nothing below waits for another wave)
    const int walker = g / shares, n0 = (g % shares) * TE_COLS;
    const int frow = lane & 31, fh = lane >> 5;
    float* st = stage_all[wave];

    uint4 b[2][KS];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int s = 0; s < KS; ++s) b[j][s] = *reinterpret_cast<const uint4*>(Wt + (size_t)(n0 + 32 * j + frow) * K + 16 * s + 8 * fh);
    const uint64_t seed_live = p > 0.0f ? live_seed(seed) : 0;   // one load of the replay-time seed word per wave
    const float inv_keep = 1.0f / (1.0f - p);
    const int nblk = (rows + TE_ROWS - 1) / TE_ROWS;
    const int lr0 = lane >> 3, c8 = lane & 7;   // the lane's stage row (+ 8 t) and 8-column chunk on the way out
    const int col0 = n0 + c8 * 8;

    auto load_a = [&](int rb, uint4 (&a)[KS]) {   // clamped row: the loads are unconditional
        const bf16_t* ap = P + (size_t)min(rb * TE_ROWS + frow, rows - 1) * K + 8 * fh;
#pragma unroll
        for (int s = 0; s < KS; ++s) a[s] = *reinterpret_cast<const uint4*>(ap + 16 * s);
    };
    // row % T of the lane's first row of a block, kept by addition: + 8 per chunk, + 32 walkers per block (one conditional subtraction
    // each, the steps being reduced mod T once: a modulo per chunk was a tenth of the kernel's instructions)
    const int step8 = 8 % T, stepw = (int)(((int64_t)walkers * TE_ROWS) % T);
    auto wrap = [&](int t) { return t - (t >= T ? T : 0); };
    float4 pb[4][2];   // the position rows of a block's 4 x 8 columns per lane (row % T < T whatever the row: no clamp)
    auto load_pb = [&](int q, int t) {
        const float* pp = posbias + (size_t)t * n + col0;
        pb[q][0] = *reinterpret_cast<const float4*>(pp);
        pb[q][1] = *reinterpret_cast<const float4*>(pp + 4);
    };
    uint4 a[KS];
    load_a(walker, a);
    int t0 = (walker * TE_ROWS + lr0) % T;
    {
        int t = t0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { load_pb(q, t); t = wrap(t + step8); }
    }
    // Loads and stores retire in issue order, so a wait for a load also waits for every store issued before it.  The block's four
    // stores are therefore held back until the NEXT block's loads are out: a (free after the MFMAs) and each chunk's position rows (free
    // after that chunk's sums).  The wait for those loads at the head of the next trip then leaves the stores in flight.
    auto block = [&](int rb, auto masked_tag) __attribute__((always_inline)) {
        constexpr bool MASKED = decltype(masked_tag)::value;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[s]), __builtin_bit_cast(bf16x8, b[j][s]), acc[j], 0, 0, 0);
        load_a(min(rb + walkers, nblk - 1), a);
        t0 = wrap(t0 + stepw);
        {
            uint4 o[4];
            int tn = t0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {   // rows 16 h .. 16 h + 15 of the block = accumulator registers 8 h .. 8 h + 7
                // C/D map of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 8; ++r) st[((r & 3) + 8 * (r >> 2) + 4 * fh) * SLD + 32 * j + frow] = acc[j][8 * h + r];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int q = 2 * h + t, lr = lr0 + 8 * t;
                    const float4 lo = *reinterpret_cast<const float4*>(st + lr * SLD + c8 * 8);
                    const float4 hi = *reinterpret_cast<const float4*>(st + lr * SLD + c8 * 8 + 4);
                    float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                    const float4 p0 = pb[q][0], p1 = pb[q][1];
                    v[0] += p0.x; v[1] += p0.y; v[2] += p0.z; v[3] += p0.w; v[4] += p1.x; v[5] += p1.y; v[6] += p1.z; v[7] += p1.w;
                    load_pb(q, tn);
                    tn = wrap(tn + step8);
                    if (p > 0.0f) {
                        // the mask of spv_dropout on the flat index of the output.  fi is a multiple of 8: the 8 columns share a 4096-block
                        // and start on an even column, so dropout_scale_at's form holds -- one hash per PAIR, the parities known at compile
                        // time (through dropout_scale hipcc, not knowing c0 even, hashed every column).  The block index is below 2^32
                        // (the host holds rows * n to 2^40), which folds the key's high-word hash into a constant of the wave.
                        const size_t fi = (size_t)(rb * TE_ROWS + lr0 + 8 * q) * n + col0;
                        const unsigned key = dropout_row_key(seed_live, (uint64_t)(unsigned)(fi >> 12));
                        const unsigned key_base = key + ((unsigned)(fi & 4095) >> 1) * 0x9e3779b1u;
#pragma unroll
                        for (int u = 0; u < 8; ++u) v[u] *= dropout_scale_at(key_base, u, p, inv_keep);
                    }
                    o[q].x = pack_bf16x2(v[0], v[1]);
                    o[q].y = pack_bf16x2(v[2], v[3]);
                    o[q].z = pack_bf16x2(v[4], v[5]);
                    o[q].w = pack_bf16x2(v[6], v[7]);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            }
            __builtin_amdgcn_sched_barrier(0);   // (the stores stay behind the loads above)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = rb * TE_ROWS + lr0 + 8 * q;
                if (!MASKED || row < rows) *reinterpret_cast<uint4*>(out + (size_t)row * n + col0) = o[q];
            }
        }
    };
    // whole blocks store without a branch (behind a branch hipcc cannot count the stores in flight and waits for ALL of them at the next
    // load it needs); the ragged last block of the tensor, which tests its rows, is the last of its walker and stands outside the loop
    const int nfull = rows / TE_ROWS;
    int rb = walker;
    for (; rb < nfull; rb += walkers) block(rb, std::false_type{});
    if (rb < nblk) block(rb, std::true_type{});
}

}  // namespace

extern "C" int spv_patchify(const float* img, void* out, int batch, int chans, int height, int width, int patch, int ld,
                            int transposed, int out_dtype, void* stream) {
    SPV_CHECK(batch > 0 && chans > 0 && patch > 0 && height >= patch && width >= patch, "spv_patchify: bad shape");
    SPV_CHECK(out_dtype == SPV_F32 || out_dtype == SPV_BF16, "spv_patchify: bad dtype");
    const int Np = (height / patch) * (width / patch), K = chans * patch * patch;
    const int64_t rows = (int64_t)batch * Np;
    SPV_CHECK(transposed >= 0 && transposed <= 2 && (transposed == 1 ? ld >= rows : ld >= K), "spv_patchify: ld=%d too small", ld);
    const int64_t total = transposed == 1 ? (int64_t)K * ld : (transposed == 2 ? (int64_t)batch * (Np + 1) * ld : rows * ld);
    if (transposed != 1 && patch % 4 == 0 && width % 4 == 0 && ld % 4 == 0 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)out & 15) == 0) {
        const int64_t vecs = (int64_t)batch * (Np + (transposed == 2 ? 1 : 0)) * (ld / 4);
        if (out_dtype == SPV_BF16)
            hipLaunchKernelGGL((patchify_vec4_kernel<bf16_t>), dim3(ew_blocks(vecs)), dim3(256), 0, static_cast<hipStream_t>(stream), img, (bf16_t*)out,
                               batch, chans, height, width, patch, ld, transposed == 2);
        else
            hipLaunchKernelGGL((patchify_vec4_kernel<float>), dim3(ew_blocks(vecs)), dim3(256), 0, static_cast<hipStream_t>(stream), img, (float*)out,
                               batch, chans, height, width, patch, ld, transposed == 2);
        SPV_LAUNCH_CHECK("spv_patchify(vec4)");
        return 0;
    }
    hipLaunchKernelGGL(patchify_kernel, dim3(ew_blocks(total)), dim3(256), 0, static_cast<hipStream_t>(stream), img, out, batch,
                       chans, height, width, patch, ld, transposed, out_dtype == SPV_BF16);
    SPV_LAUNCH_CHECK("spv_patchify");
    return 0;
}

extern "C" int spv_patchify_u8(const unsigned char* img_hwc, const float* mean, const float* inv_std, void* out, int batch,
                               int chans, int height, int width, int patch, int ld, int transposed, int out_dtype, void* stream) {
    SPV_CHECK(batch > 0 && chans > 0 && patch > 0 && height >= patch && width >= patch, "spv_patchify_u8: bad shape");
    SPV_CHECK(out_dtype == SPV_F32 || out_dtype == SPV_BF16, "spv_patchify_u8: bad dtype");
    SPV_CHECK(mean != nullptr && inv_std != nullptr, "spv_patchify_u8: mean / inv_std missing");
    const int Np = (height / patch) * (width / patch), K = chans * patch * patch;
    const int64_t rows = (int64_t)batch * Np;
    SPV_CHECK(transposed >= 0 && transposed <= 2 && (transposed == 1 ? ld >= rows : ld >= K), "spv_patchify_u8: ld=%d too small", ld);
    const int64_t total = transposed == 1 ? (int64_t)K * ld : (transposed == 2 ? (int64_t)batch * (Np + 1) * ld : rows * ld);
    hipLaunchKernelGGL(patchify_u8_kernel, dim3(ew_blocks(total)), dim3(256), 0, static_cast<hipStream_t>(stream), img_hwc, mean,
                       inv_std, out, batch, chans, height, width, patch, ld, transposed, out_dtype == SPV_BF16);
    SPV_LAUNCH_CHECK("spv_patchify_u8");
    return 0;
}

extern "C" int spv_embed_posbias(const float* pos, const float* bias, const float* cls, float* out, int patches, int embed, void* stream) {
    SPV_CHECK(patches > 0 && embed > 0, "spv_embed_posbias: empty");
    hipLaunchKernelGGL(posbias_kernel, dim3(ew_blocks((int64_t)(patches + 1) * embed)), dim3(256), 0, static_cast<hipStream_t>(stream), pos,
                       bias, cls, out, patches, embed);
    SPV_LAUNCH_CHECK("spv_embed_posbias");
    return 0;
}

extern "C" int spv_embed_cls_rows(const float* cls, const float* pos, void* tokens, int batch, int tokens_per_image, int embed,
                                  int dtype, void* stream) {
    SPV_CHECK(batch > 0 && tokens_per_image > 0 && embed > 0, "spv_embed_cls_rows: empty");
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_embed_cls_rows: bad dtype");
    hipLaunchKernelGGL(cls_rows_kernel, dim3(ew_blocks((int64_t)batch * embed)), dim3(256), 0, static_cast<hipStream_t>(stream), cls,
                       pos, tokens, batch, tokens_per_image, embed, dtype == SPV_BF16);
    SPV_LAUNCH_CHECK("spv_embed_cls_rows");
    return 0;
}

extern "C" int spv_token_embed_supported(int rows, int n, int k, int dtype) { return token_embed_supported(rows, n, k, dtype); }

extern "C" int spv_token_embed_fwd(const void* patches, const void* w, const float* posbias, void* tokens, int rows, int n, int k,
                                   int tokens_per_image, float p_drop, uint64_t seed, void* stream) {
    SPV_CHECK(token_embed_supported(rows, n, k, SPV_BF16) && (int64_t)rows * n <= (1ll << 40),
              "spv_token_embed_fwd: unsupported shape %d x %d x %d (bf16; k a multiple of 16 in 16..64; n a multiple of 64; rows * n <= 2^40)", rows, n, k);
    SPV_CHECK(tokens_per_image > 0, "spv_token_embed_fwd: tokens_per_image=%d", tokens_per_image);
    SPV_CHECK(p_drop >= 0.0f && p_drop < 1.0f, "spv_token_embed_fwd: p_drop=%f", p_drop);
    SPV_CHECK(patches && w && posbias && tokens, "spv_token_embed_fwd: null pointer");
    SPV_CHECK((((uintptr_t)patches | (uintptr_t)w | (uintptr_t)posbias | (uintptr_t)tokens) & 15) == 0,
              "spv_token_embed_fwd: pointers must be 16-byte aligned");
    static int cus = 0;   // (every device of a process is the same part)
    if (cus == 0) {
        int dev = 0, v = 0;
        SPV_CHECK(hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0,
                  "spv_token_embed_fwd: no device to size the grid for");
        cus = v;
    }
    const TokenEmbedPlan pl = token_embed_plan(rows, n, cus);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define SPV_TOKEN_EMBED(KS)                                                                                                      \
    hipLaunchKernelGGL((token_embed_kernel<KS>), dim3(pl.grid), dim3(64 * TE_WAVES), 0, st, static_cast<const bf16_t*>(patches), \
                       static_cast<const bf16_t*>(w), posbias, static_cast<bf16_t*>(tokens), rows, n, tokens_per_image, pl.shares, \
                       pl.walkers, p_drop, seed)
    switch (k / 16) {
    case 1: SPV_TOKEN_EMBED(1); break;
    case 2: SPV_TOKEN_EMBED(2); break;
    case 3: SPV_TOKEN_EMBED(3); break;
    default: SPV_TOKEN_EMBED(4); break;
    }
#undef SPV_TOKEN_EMBED
    SPV_LAUNCH_CHECK("spv_token_embed_fwd");
    return 0;
}

// ---- backward of the token tensor, one pass: dtok = dropout_mask(g [+ gcls on the CLS rows]) and the column sums over the batch
// that the position / bias / class-token gradients are made of.  (Separately this was a strided add, a dropout pass, a column-sum
// pass and three small folds over a 34 MB tensor: seven launches.)  grid = (column blocks of 8-element vectors, groups of EB_GS samples).
constexpr int EB_GS = 16, EB_HB = 8;   // samples per workgroup row-group; loads in flight per thread
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_rows_kernel(const T* __restrict__ g, const T* __restrict__ gcls, T* __restrict__ dtok,
                                                            float* __restrict__ partials, int B, int TE, int E, float p, uint64_t seed) {
    const int v = blockIdx.x * 256 + threadIdx.x;          // 8-element vector of the [T * E] row
    if (v * 8 >= TE) return;
    const int col = v * 8;
    const int b0 = blockIdx.y * EB_GS;
    const float inv_keep = 1.0f / (1.0f - p);
    const uint64_t sd = live_seed(seed);
    float acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.0f;
    const bool cls_row = gcls != nullptr && col < E;
    if constexpr (sizeof(T) == 2) {
        // bf16: one 16-byte load per row (two 8-byte loads were half the bytes per request)
        typedef unsigned raw4 __attribute__((ext_vector_type(4)));
        // (EB_HB rows at a time: < 128 VGPRs, so that this 256-thread workgroup fits on a CU BESIDE a workgroup of the batched weight
        // gradients -- 8 waves x 184 VGPRs leave 144 per SIMD -- which is where it runs: at 145 it waited for that kernel's CUs to drain)
        for (int h0 = 0; h0 < EB_GS; h0 += EB_HB) {
            raw4 xr[EB_HB], cr[EB_HB];
#pragma unroll
            for (int s = 0; s < EB_HB; ++s) xr[s] = *reinterpret_cast<const raw4*>(g + (size_t)min(b0 + h0 + s, B - 1) * TE + col);
            if (cls_row) {   // (one workgroup of the grid's column blocks)
#pragma unroll
                for (int s = 0; s < EB_HB; ++s) cr[s] = *reinterpret_cast<const raw4*>(gcls + (size_t)min(b0 + h0 + s, B - 1) * E + col);
            }
#pragma unroll
            for (int s = 0; s < EB_HB; ++s) {
                const int b = b0 + h0 + s;
                if (b >= B) break;
                const size_t i = (size_t)b * TE + col;
                float x[8];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    x[2 * u] = __uint_as_float(xr[s][u] << 16);
                    x[2 * u + 1] = __uint_as_float(xr[s][u] & 0xffff0000u);
                }
                if (cls_row) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        x[2 * u] += __uint_as_float(cr[s][u] << 16);
                        x[2 * u + 1] += __uint_as_float(cr[s][u] & 0xffff0000u);
                    }
                }
                if (p > 0.0f) {
                    const unsigned key = dropout_row_key(sd, (uint64_t)i >> 12);
                    const unsigned c0 = (unsigned)(i & 4095);
#pragma unroll
                    for (int u = 0; u < 8; ++u) x[u] *= dropout_scale(key, c0 + u, p, inv_keep);
                }
                raw4 o;
#pragma unroll
                for (int u = 0; u < 4; ++u) o[u] = pack_bf16x2(x[2 * u], x[2 * u + 1]);
                if (dtok != nullptr) *reinterpret_cast<raw4*>(dtok + i) = o;
#pragma unroll
                for (int u = 0; u < 4; ++u) {   // the sums are taken over what the weight-gradient GEMM reads: the rounded values
                    acc[2 * u] += __uint_as_float(o[u] << 16);
                    acc[2 * u + 1] += __uint_as_float(o[u] & 0xffff0000u);
                }
            }
        }
    } else {
    // EB_HB rows' loads are issued before the first is used (clamped addresses, masked sums): one row per trip was a chain of HBM
    // round trips (25 us for 68 MB)
    for (int h0 = 0; h0 < EB_GS; h0 += EB_HB) {
        float x[EB_HB][8], c[EB_HB][8];
#pragma unroll
        for (int s = 0; s < EB_HB; ++s) {
            const int b = min(b0 + h0 + s, B - 1);
            const size_t i = (size_t)b * TE + col;
            io<T>::ld4(g + i, *reinterpret_cast<float(*)[4]>(&x[s][0]));
            io<T>::ld4(g + i + 4, *reinterpret_cast<float(*)[4]>(&x[s][4]));
            if (cls_row) {   // block-uniform for all but one block
                io<T>::ld4(gcls + (size_t)b * E + col, *reinterpret_cast<float(*)[4]>(&c[s][0]));
                io<T>::ld4(gcls + (size_t)b * E + col + 4, *reinterpret_cast<float(*)[4]>(&c[s][4]));
            }
        }
#pragma unroll
        for (int s = 0; s < EB_HB; ++s) {
            const int b = b0 + h0 + s;
            if (b >= B) break;
            const size_t i = (size_t)b * TE + col;
            if (cls_row) {
#pragma unroll
                for (int u = 0; u < 8; ++u) x[s][u] += c[s][u];
            }
            if (p > 0.0f) {
                const unsigned key = dropout_row_key(sd, (uint64_t)i >> 12);
                const unsigned c0 = (unsigned)(i & 4095);
#pragma unroll
                for (int u = 0; u < 8; ++u) x[s][u] *= dropout_scale(key, c0 + u, p, inv_keep);
            }
            if (dtok != nullptr) {
                io<T>::st4(dtok + i, *reinterpret_cast<const float(*)[4]>(&x[s][0]));
                io<T>::st4(dtok + i + 4, *reinterpret_cast<const float(*)[4]>(&x[s][4]));
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += x[s][u];
        }
    }
    }
    float* po = partials + (size_t)blockIdx.y * TE + col;
    *reinterpret_cast<float4*>(po) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(po + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// dpos[t][e] = sum_groups partials; dcls[e] = dpos[0][e]: one column of the flat [T * E] row per thread, its `groups` partials as
// independent loads, 256-thread workgroups with few registers -- they run on CUs that the batched weight gradients occupy (one
// 1024-thread workgroup per 16 columns, E / 16 = 32 of them reading 64-byte half lines, took 73-104 us there and held up the embedding
// weight gradient behind it on the main stream; so did 1024-thread workgroups of any shape: 16 waves do not fit beside that kernel).
// dbias[e] = sum_{t >= 1} dpos[t][e] follows as a launch of its own (E / 64 single-wave workgroups over 133 KB that are still in L2).
constexpr int EF_T = 256;
__global__ __launch_bounds__(EF_T) void embed_bwd_fold_kernel(const float* __restrict__ partials, float* __restrict__ dpos, float* __restrict__ dcls,
                                                             int groups, int TE, int E) {
    const int c = blockIdx.x * EF_T + threadIdx.x;
    if (c >= TE) return;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int g = 0;
    for (; g + 8 <= groups; g += 8) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = partials[(size_t)(g + u) * TE + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u & 3] += q[u];
    }
    for (; g < groups; ++g) a[0] += partials[(size_t)g * TE + c];
    const float v = (a[0] + a[1]) + (a[2] + a[3]);
    dpos[c] = v;
    if (c < E) dcls[c] = v;
}
__global__ __launch_bounds__(64) void embed_bwd_bias_kernel(const float* __restrict__ dpos, float* __restrict__ dbias, int T, int E) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int t = 1;
    for (; t + 8 <= T; t += 8) {
        float q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) q[u] = dpos[(size_t)(t + u) * E + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u & 3] += q[u];
    }
    for (; t < T; ++t) a[0] += dpos[(size_t)t * E + e];
    dbias[e] = (a[0] + a[1]) + (a[2] + a[3]);
}

extern "C" int spv_embed_bwd_groups(int batch) { return cdiv(batch, EB_GS); }

extern "C" int spv_embed_bwd(const void* g, const void* gcls, void* dtok, float* partials, float* dpos, float* dbias, float* dcls, int batch,
                             int tokens, int embed, float p_drop, uint64_t seed, int dtype, void* stream) {
    SPV_CHECK(batch > 0 && tokens > 0 && embed > 0 && embed % 8 == 0, "spv_embed_bwd: bad shape %d x %d x %d (embed must be a multiple of 8)", batch, tokens, embed);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_embed_bwd: bad dtype");
    SPV_CHECK(p_drop >= 0.0f && p_drop < 1.0f, "spv_embed_bwd: p_drop=%f", p_drop);
    SPV_CHECK(g && partials && dpos && dbias && dcls, "spv_embed_bwd: null pointer");
    SPV_CHECK(dtok != nullptr || (gcls == nullptr && p_drop == 0.0f), "spv_embed_bwd: dtok may be NULL only when it would equal g");
    SPV_CHECK((int64_t)tokens * embed < (1ll << 28), "spv_embed_bwd: row too long");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int TE = tokens * embed, groups = cdiv(batch, EB_GS);
    const dim3 grid(cdiv(TE / 8, 256), groups);
    if (dtype == SPV_BF16)
        hipLaunchKernelGGL((embed_bwd_rows_kernel<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)g, (const bf16_t*)gcls, (bf16_t*)dtok, partials, batch, TE,
                           embed, p_drop, seed);
    else
        hipLaunchKernelGGL((embed_bwd_rows_kernel<float>), grid, dim3(256), 0, st, (const float*)g, (const float*)gcls, (float*)dtok, partials, batch, TE, embed,
                           p_drop, seed);
    SPV_LAUNCH_CHECK("spv_embed_bwd(rows)");
    hipLaunchKernelGGL(embed_bwd_fold_kernel, dim3(cdiv(TE, EF_T)), dim3(EF_T), 0, st, partials, dpos, dcls, groups, TE, embed);
    hipLaunchKernelGGL(embed_bwd_bias_kernel, dim3(cdiv(embed, 64)), dim3(64), 0, st, dpos, dbias, tokens, embed);
    SPV_LAUNCH_CHECK("spv_embed_bwd(fold)");
    return 0;
}

extern "C" int spv_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, int dtype, void* stream) {
    SPV_CHECK(p >= 0.0f && p < 1.0f, "spv_dropout: p=%f", p);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_dropout: bad dtype");
    if (n <= 0) return 0;
    SPV_CHECK(((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0, "spv_dropout: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(dropout_kernel, dim3(ew_blocks((n + 7) / 8)), dim3(256), 0, static_cast<hipStream_t>(stream), x, y, n, p, seed,
                       dtype == SPV_BF16);
    SPV_LAUNCH_CHECK("spv_dropout");
    return 0;
}

extern "C" int spv_spectral_fold(const float* proj_w, const float* freq_h, const float* freq_w, float* w_full, int embed, int chans,
                                 int patch, void* stream) {
    SPV_CHECK(embed > 0 && chans > 0 && patch > 0, "spv_spectral_fold: empty");
    hipLaunchKernelGGL(spectral_fold_kernel, dim3(ew_blocks((int64_t)embed * chans * patch * patch)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), proj_w, freq_h, freq_w, w_full, embed, chans, patch);
    SPV_LAUNCH_CHECK("spv_spectral_fold");
    return 0;
}

extern "C" int spv_spectral_fold_bf16(const float* proj_w, const float* freq_h, const float* freq_w, float* w_full, void* w_full_bf16, int embed,
                                      int chans, int patch, void* stream) {
    SPV_CHECK(embed > 0 && chans > 0 && patch > 0 && w_full_bf16 != nullptr, "spv_spectral_fold_bf16: bad arguments");
    hipLaunchKernelGGL(spectral_fold_kernel, dim3(ew_blocks((int64_t)embed * chans * patch * patch)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), proj_w, freq_h, freq_w, w_full, embed, chans, patch, static_cast<bf16_t*>(w_full_bf16));
    SPV_LAUNCH_CHECK("spv_spectral_fold_bf16");
    return 0;
}

// scratch: fp32, embed * chans * patch * (patch/2+1) floats
extern "C" int spv_spectral_fold_bwd(const float* dw_full, const float* proj_w, const float* freq_h, const float* freq_w,
                                     float* dproj_w, float* dfreq_h, float* dfreq_w, float* scratch, int embed, int chans, int patch,
                                     void* stream) {
    SPV_CHECK(embed > 0 && chans > 0 && patch > 0 && patch <= 64, "spv_spectral_fold_bwd: bad shape");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Pv = patch / 2 + 1;
    hipLaunchKernelGGL(spectral_fold_bwd_kernel, dim3(ew_blocks((int64_t)embed * chans * patch * Pv)), dim3(256), 0, st, dw_full,
                       proj_w, freq_h, freq_w, dproj_w, scratch, embed, chans, patch);
    SPV_LAUNCH_CHECK("spv_spectral_fold_bwd");
    int nt = 1024;   // rows of [patch + Pv] floats within 48 KiB of LDS
    while (nt > 64 && (size_t)nt * (patch + Pv) * sizeof(float) > 48 * 1024) nt >>= 1;
    SPV_CHECK((size_t)nt * (patch + Pv) * sizeof(float) <= 64 * 1024, "spv_spectral_fold_bwd: patch %d too large", patch);
    hipLaunchKernelGGL(freq_weight_grad_kernel, dim3(1), dim3(nt), (size_t)nt * (patch + Pv) * sizeof(float), st, scratch, freq_h,
                       freq_w, dfreq_h, dfreq_w, embed * chans, patch);
    SPV_LAUNCH_CHECK("spv_spectral_fold_bwd(freq)");
    return 0;
}

int spv_seed_ptr_set_patch(const unsigned long long* p) { return spv_seed_symbol_set(p); }
