// Training augmentation on the device: the transform chain of the reference's loader (spectre_vit/repl/train.py:100-115,
// RandomHorizontalFlip -> ColorJitter -> RandomGrayscale -> RandomAffine -> RandomApply([GaussianBlur(3)]) -> ToTensor -> Normalize ->
// RandomErasing) as two kernels: spv_augment_params draws the per-sample parameter table, spv_augment_u8 applies it, one workgroup per
// image with the image staged in LDS.  Definitions: include/spv.h and DESIGN.md section 4c.  At the end of the file the resident
// loader's fetch, the draw and the chain as ONE kernel that reads the step from the loader's device cursor (spv_loader_fetch_augment,
// DESIGN.md section 4k): draw and chain are device functions with one definition each, called from both places.
#include "spv_common.h"
#include "spv_augment_core.h"   // clamp01, grey_of, hue_shift: shared with the tiled kernels
#include "spv_augment_draw.h"   // the draw of a table row and its host checks: shared with the fused tiled fetch
#include "spv_loader_core.h"    // the fused fetch at the end of this file: the sample order and the cursor's protocol
#include <math.h>

constexpr int AUG_THREADS = 256;
constexpr int AUG_WAVES = AUG_THREADS / 64;
static_assert(AUG_WAVES == 4, "the contrast mean adds four per-wave partial sums");
constexpr int AUG_LDS_BYTES = 64 * 1024;   // what a workgroup may take without an opt-in attribute
constexpr int AUG_RED_FLOATS = 8;          // per-wave partial sums of the contrast mean

static inline size_t aug_lds_bytes(int chans, int height, int width) {
    return ((size_t)2 * chans * height * width + AUG_RED_FLOATS) * sizeof(float);
}

extern "C" int spv_augment_supported(int chans, int height, int width) {
    if (!(chans == 1 || chans == 3) || height < 2 || width < 2 || height > 4096 || width > 4096) return 0;
    return aug_lds_bytes(chans, height, width) <= (size_t)AUG_LDS_BYTES ? 1 : 0;
}

// the fused fetch keeps, behind the chain's floats, what its workgroup hands from one thread to the others: the sample's table row,
// the step (64 bits) and the row of the set, padded to 16 bytes
constexpr int FUSED_TAIL_FLOATS = SPV_AUG_NPARAM + 4;
static inline size_t fused_lds_bytes(int chans, int height, int width) {
    return aug_lds_bytes(chans, height, width) + FUSED_TAIL_FLOATS * sizeof(float);
}

extern "C" int spv_loader_augment_supported(int chans, int height, int width) {
    if (!spv_augment_supported(chans, height, width) || height > 512 || width > 512) return 0;   // the chain's shapes that the loader takes
    return fused_lds_bytes(chans, height, width) <= (size_t)AUG_LDS_BYTES ? 1 : 0;
}

// ---------------------------------------------------------------- parameter draws (the draw itself: spv_augment_draw.h)
__global__ __launch_bounds__(AUG_THREADS) void augment_params_kernel(float* __restrict__ params, int B, int H, int W, spv_augment_cfg c,
                                                                     uint64_t seed, uint64_t step) {
    const int s = blockIdx.x * AUG_THREADS + threadIdx.x;
    if (s >= B) return;
    aug_store_row(params, (unsigned)s, aug_draw(H, W, c, seed, step, (unsigned)s));
}

extern "C" int spv_augment_params(float* params, int batch, int chans, int height, int width, const spv_augment_cfg* cfg, uint64_t seed,
                                  uint64_t step, void* stream) {
    if (int rc = aug_draw_check("spv_augment_params", params, cfg, batch, chans, height, width)) return rc;
    const spv_augment_cfg& c = *cfg;
    hipLaunchKernelGGL(augment_params_kernel, dim3(cdiv(batch, AUG_THREADS)), dim3(AUG_THREADS), 0, static_cast<hipStream_t>(stream), params,
                       batch, height, width, c, seed, step);
    SPV_LAUNCH_CHECK("spv_augment_params");
    return 0;
}

// ---------------------------------------------------------------- the chain
// LDS: two planar [C][H][W] fp32 images (12 KiB each at 3 x 32 x 32) + the reduction slots.  Planar, so that the per-pixel passes touch
// consecutive addresses per channel (no bank conflict) and the result leaves as it lies (NCHW).  The rotation's gather reads address
// sy * W + sx: at W = 32 and |angle| <= 30 degrees two lanes of a 32-lane group (one output row) meet on a bank only with equal sx and
// sy two rows apart, which needs >= 4 pixels along the row (sin 30 = 0.5) over which sx has moved by >= 3 (cos 30 = 0.87): conflict free.
// Thread t owns pixels t, t + 256, ... through the jitter and grayscale ops (no barrier between them; the contrast mean is the one
// workgroup reduction); rotation and blur read neighbours, with a barrier in front of each pass.
template <int C>
__device__ __forceinline__ void aug_chain(const unsigned char* __restrict__ img, const AugRow row, float* __restrict__ o, float* lds,
                                          const float* __restrict__ mean, const float* __restrict__ inv_std, int H, int W, int vec) {
    const int HW = H * W, CHW = C * HW;
    float* cur = lds;
    float* oth = lds + CHW;
    float* red = lds + 2 * CHW;
    const int tid = threadIdx.x;
    const float* p = row.v;

    // 1. load u8 / 255, mirrored in W if flip: the owner of output pixel (y, x) reads source pixel (y, W - 1 - x)
    const bool flip = p[SPV_AUG_FLIP] != 0.0f;
    for (int px = tid; px < HW; px += AUG_THREADS) {
        const int y = px / W, x = px - y * W;
        const unsigned char* s = img + (size_t)(y * W + (flip ? W - 1 - x : x)) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) cur[c * HW + px] = (float)s[c] / 255.0f;
    }

    // 2. ColorJitter: the four ops in the order the permutation index names (lexicographic over b, c, s, h = 0, 1, 2, 3)
    {
        int idx = (int)p[SPV_AUG_ORDER];
        idx = idx < 0 ? 0 : (idx > 23 ? 23 : idx);
        unsigned avail = 0x3210u;   // the ops not yet used, one per nibble, ascending
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int n = k == 0 ? idx / 6 : (k == 1 ? (idx % 6) / 2 : (k == 2 ? idx % 2 : 0));
            const int op = (int)((avail >> (4 * n)) & 0xfu);
            avail = (avail & ((1u << (4 * n)) - 1u)) | ((avail >> (4 * n + 4)) << (4 * n));
            if (op == 0) {
                const float f = p[SPV_AUG_BRIGHT];
                for (int px = tid; px < HW; px += AUG_THREADS) {
#pragma unroll
                    for (int c = 0; c < C; ++c) cur[c * HW + px] = clamp01(cur[c * HW + px] * f);
                }
            } else if (op == 1) {
                const float f = p[SPV_AUG_CONTRAST];
                float part = 0.0f;
                for (int px = tid; px < HW; px += AUG_THREADS) {
                    if constexpr (C == 3) part += grey_of(cur[px], cur[HW + px], cur[2 * HW + px]);
                    else part += cur[px];
                }
                part = wave_sum(part);
                if ((tid & 63) == 0) red[tid >> 6] = part;
                __syncthreads();
                const float m = ((red[0] + red[1]) + (red[2] + red[3])) / (float)HW;
                const float add = (1.0f - f) * m;
                for (int px = tid; px < HW; px += AUG_THREADS) {
#pragma unroll
                    for (int c = 0; c < C; ++c) cur[c * HW + px] = clamp01(f * cur[c * HW + px] + add);
                }
            } else if (op == 2) {
                if constexpr (C == 3) {
                    const float f = p[SPV_AUG_SAT];
                    for (int px = tid; px < HW; px += AUG_THREADS) {
                        const float r = cur[px], g = cur[HW + px], bl = cur[2 * HW + px];
                        const float gr = (1.0f - f) * grey_of(r, g, bl);
                        cur[px] = clamp01(f * r + gr);
                        cur[HW + px] = clamp01(f * g + gr);
                        cur[2 * HW + px] = clamp01(f * bl + gr);
                    }
                }
            } else {
                if constexpr (C == 3) {
                    const float shift = p[SPV_AUG_HUE];
                    if (shift != 0.0f) {
                        for (int px = tid; px < HW; px += AUG_THREADS) {
                            float r = cur[px], g = cur[HW + px], bl = cur[2 * HW + px];
                            hue_shift(r, g, bl, shift);
                            cur[px] = r;
                            cur[HW + px] = g;
                            cur[2 * HW + px] = bl;
                        }
                    }
                }
            }
        }
    }

    // 3. grayscale
    if constexpr (C == 3) {
        if (p[SPV_AUG_GRAY] != 0.0f) {
            for (int px = tid; px < HW; px += AUG_THREADS) {
                const float gr = grey_of(cur[px], cur[HW + px], cur[2 * HW + px]);
                cur[px] = gr;
                cur[HW + px] = gr;
                cur[2 * HW + px] = gr;
            }
        }
    }

    // 4. rotation: nearest neighbour through the inverse map torchvision hands to PIL, zero fill
    const float angle = p[SPV_AUG_ANGLE];
    if (angle != 0.0f) {
        __syncthreads();
        const float rad = -angle * 0.017453292519943295f;
        const float cs = cosf(rad), sn = sinf(rad);
        const float cx = 0.5f * (float)W, cy = 0.5f * (float)H;
        const float tx = cx - cx * cs - cy * sn, ty = cy + cx * sn - cy * cs;
        for (int px = tid; px < HW; px += AUG_THREADS) {
            const int y = px / W, x = px - y * W;
            const float X = (float)x + 0.5f, Y = (float)y + 0.5f;
            const float sx = cs * X + sn * Y + tx, sy = -sn * X + cs * Y + ty;
            const int ix = (int)floorf(sx), iy = (int)floorf(sy);
            const bool in = ix >= 0 && ix < W && iy >= 0 && iy < H;
            const int sp = in ? iy * W + ix : 0;
#pragma unroll
            for (int c = 0; c < C; ++c) oth[c * HW + px] = in ? cur[c * HW + sp] : 0.0f;
        }
        float* t = cur; cur = oth; oth = t;
    }

    // 5. blur: separable 3 taps, reflect padding (index -1 -> 1, W -> W - 2)
    if (p[SPV_AUG_BLUR] != 0.0f) {
        const float sigma = p[SPV_AUG_SIGMA];
        const float e = expf(-1.0f / (2.0f * sigma * sigma));
        const float norm = 1.0f + 2.0f * e;
        const float w0 = 1.0f / norm, w1 = e / norm;
        __syncthreads();
        for (int px = tid; px < HW; px += AUG_THREADS) {
            const int y = px / W, x = px - y * W;
            const int xl = x == 0 ? 1 : x - 1, xr = x == W - 1 ? W - 2 : x + 1;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float* r = cur + c * HW + y * W;
                oth[c * HW + px] = w1 * r[xl] + w0 * r[x] + w1 * r[xr];
            }
        }
        __syncthreads();
        for (int px = tid; px < HW; px += AUG_THREADS) {
            const int y = px / W, x = px - y * W;
            const int yu = y == 0 ? 1 : y - 1, yd = y == H - 1 ? H - 2 : y + 1;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float* pl = oth + c * HW;
                cur[c * HW + px] = w1 * pl[yu * W + x] + w0 * pl[px] + w1 * pl[yd * W + x];
            }
        }
    }
    __syncthreads();

    // 6. + 7. normalise, erase, store NCHW (the LDS image is the output's layout)
    const int ei = (int)p[SPV_AUG_ERASE_I], ej = (int)p[SPV_AUG_ERASE_J];
    const int eh = (int)p[SPV_AUG_ERASE_H], ew = (int)p[SPV_AUG_ERASE_W];
    if (vec) {   // HW % 4 == 0 and out 16-byte aligned: a float4 lies inside one channel plane
        for (int q = tid; q < CHW / 4; q += AUG_THREADS) {
            const int e0 = 4 * q;
            const int c = e0 / HW, px = e0 - c * HW;
            const float mu = mean[c], is = inv_std[c];
            const float4 v = *reinterpret_cast<const float4*>(cur + e0);
            float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int y = (px + u) / W, x = (px + u) - y * W;
                const bool erased = y >= ei && y < ei + eh && x >= ej && x < ej + ew;
                r[u] = erased ? 0.0f : (r[u] - mu) * is;
            }
            *reinterpret_cast<float4*>(o + e0) = make_float4(r[0], r[1], r[2], r[3]);
        }
    } else {
        for (int e = tid; e < CHW; e += AUG_THREADS) {
            const int c = e / HW, px = e - c * HW;
            const int y = px / W, x = px - y * W;
            const bool erased = y >= ei && y < ei + eh && x >= ej && x < ej + ew;
            o[e] = erased ? 0.0f : (cur[e] - mean[c]) * inv_std[c];
        }
    }
}

template <int C>
__global__ __launch_bounds__(AUG_THREADS) void augment_u8_kernel(const unsigned char* __restrict__ src, const int64_t* __restrict__ index,
                                                                 const float* __restrict__ params, const float* __restrict__ mean,
                                                                 const float* __restrict__ inv_std, float* __restrict__ out, int n_src,
                                                                 int H, int W, int vec) {
    extern __shared__ float lds[];
    const int CHW = C * H * W;
    const int b = blockIdx.x, tid = threadIdx.x;
    float* o = out + (size_t)b * CHW;
    const int64_t row = index != nullptr ? index[b] : (int64_t)b;
    if (row < 0 || row >= (int64_t)n_src) {   // workgroup uniform: nothing is read, the image is poisoned
        for (int e = tid; e < CHW; e += AUG_THREADS) o[e] = __builtin_nanf("");
        return;
    }
    AugRow r;
#pragma unroll
    for (int i = 0; i < SPV_AUG_NPARAM; ++i) r.v[i] = params[(size_t)b * SPV_AUG_NPARAM + i];
    aug_chain<C>(src + (size_t)row * CHW, r, o, lds, mean, inv_std, H, W, vec);
}

extern "C" int spv_augment_u8(const unsigned char* src_nhwc, const int64_t* index, const float* params, const float* mean,
                              const float* inv_std, float* out_nchw, int batch, int n_src, int chans, int height, int width, void* stream) {
    SPV_CHECK(batch > 0 && n_src > 0 && chans > 0 && height > 0 && width > 0, "spv_augment_u8: bad shape");
    SPV_CHECK(spv_augment_supported(chans, height, width),
              "spv_augment_u8: a %d x %d x %d image is not supported (1 or 3 channels, two fp32 copies of the image within %d bytes of LDS)",
              chans, height, width, AUG_LDS_BYTES);
    SPV_CHECK(src_nhwc != nullptr && out_nchw != nullptr, "spv_augment_u8: src / out missing");
    SPV_CHECK(params != nullptr, "spv_augment_u8: params missing");
    SPV_CHECK(mean != nullptr && inv_std != nullptr, "spv_augment_u8: mean / inv_std missing");
    SPV_CHECK(index != nullptr || batch <= n_src, "spv_augment_u8: index == NULL reads rows 0..batch-1, but batch=%d > n_src=%d", batch, n_src);
    SPV_CHECK(((uintptr_t)out_nchw & 3) == 0 && ((uintptr_t)params & 3) == 0, "spv_augment_u8: out / params must be 4-byte aligned");
    const int vec = (height * width) % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0;
    const size_t lds = aug_lds_bytes(chans, height, width);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (chans == 3)
        hipLaunchKernelGGL(augment_u8_kernel<3>, dim3(batch), dim3(AUG_THREADS), lds, st, src_nhwc, index, params, mean, inv_std, out_nchw,
                           n_src, height, width, vec);
    else
        hipLaunchKernelGGL(augment_u8_kernel<1>, dim3(batch), dim3(AUG_THREADS), lds, st, src_nhwc, index, params, mean, inv_std, out_nchw,
                           n_src, height, width, vec);
    SPV_LAUNCH_CHECK("spv_augment_u8");
    SPV_COUNT_PATH(SPV_PATH_AUGMENT);
    return 0;
}

// ---------------------------------------------------------------- fetch and augment in one launch
// spv_loader_fetch(mode none) at the cursor's step t, spv_augment_params(step = t) and spv_augment_u8 as ONE launch, one workgroup per
// image: nothing of it is a by-value function of the step, so a captured launch draws a new batch AND a new table at every replay.
struct FusedArgs {
    const unsigned char* src;     // [n][H][W][C]
    const void* labels_src;       // [n] uint8 or int64
    unsigned long long* cursor;   // the loader's cursor block
    int64_t* index;               // [batch]
    int64_t* labels;              // [batch]
    float* params;                // [batch][16]
    float* out;                   // [batch][C][H][W]
    const float* mean;
    const float* inv_std;
    uint64_t loader_seed, augment_seed;
    LdrGeom g;
    spv_augment_cfg cfg;
    int H, W, vec, label_i64;
};

// Thread 0 reads the step and hands it round; then the row of the set (wave 0) and the table row (wave 1) -- both functions of (t, b)
// alone -- are worked out side by side and handed round through LDS (never through `params` in global memory: a line of it cached
// from the previous replay may be stale in this CU's vector cache), and wave 2 takes the workgroup's ticket while the others already
// load the image.  The ticket comes after the read of t in every workgroup, which is all the protocol asks: the last workgroup to
// arrive knows that every other one holds its copy of t, and only then stores t + 1.
template <int C>
__global__ __launch_bounds__(AUG_THREADS) void loader_augment_kernel(FusedArgs a) {
    extern __shared__ float lds[];
    const int CHW = C * a.H * a.W;
    float* row_sh = lds + 2 * CHW + AUG_RED_FLOATS;                                               // [16]
    unsigned long long* t_sh = reinterpret_cast<unsigned long long*>(row_sh + SPV_AUG_NPARAM);   // 8-byte aligned: 8 CHW + 96 bytes in
    uint32_t* idx_sh = reinterpret_cast<uint32_t*>(t_sh + 1);
    const uint32_t b = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) *t_sh = ldr_read_step(a.cursor);
    __syncthreads();
    const uint64_t t = *t_sh;
    if (tid == 0) {
        const uint32_t idx = ldr_index(a.loader_seed, t, b, a.g);
        a.index[b] = (int64_t)idx;
        a.labels[b] = a.label_i64 ? static_cast<const int64_t*>(a.labels_src)[idx]
                                  : (int64_t) static_cast<const unsigned char*>(a.labels_src)[idx];
        *idx_sh = idx;
    } else if (tid == 64) {
        const AugRow r = aug_draw(a.H, a.W, a.cfg, a.augment_seed, t, b);
        aug_store_row(a.params, b, r);
#pragma unroll
        for (int i = 0; i < SPV_AUG_NPARAM; ++i) row_sh[i] = r.v[i];
    }
    __syncthreads();
    if (tid == 128) ldr_arrive<false>(a.cursor, t, a.g.batch);   // groups = batch; t came through LDS behind two barriers: the read is done
    AugRow r;
#pragma unroll
    for (int i = 0; i < SPV_AUG_NPARAM; ++i) r.v[i] = row_sh[i];
    const uint32_t idx = *idx_sh;   // < n by construction (spv_loader_core.h)
    aug_chain<C>(a.src + (size_t)idx * CHW, r, a.out + (size_t)b * CHW, lds, a.mean, a.inv_std, a.H, a.W, a.vec);
}

extern "C" int spv_loader_fetch_augment(const unsigned char* src_nhwc, const void* labels_src, void* cursor, int64_t* index, int64_t* labels,
                                        float* params, float* out_nchw, const float* mean, const float* inv_std,
                                        const spv_augment_cfg* cfg, int n, int batch, int chans, int height, int width, int world, int rank,
                                        int steps_per_epoch, uint64_t loader_seed, int shuffle, int label_dtype, uint64_t augment_seed,
                                        void* stream) {
    const char* name = "spv_loader_fetch_augment";
    // the fetch's refusals (as its float mode: src, img, mean and inv_std are all read), then the draw's, then this kernel's own
    if (int rc = spv_loader_check(name, src_nhwc, labels_src, cursor, index, labels, out_nchw, mean, inv_std, n, batch, chans, height, width,
                                  world, rank, steps_per_epoch, SPV_LOADER_FLOAT, label_dtype))
        return rc;
    if (int rc = aug_draw_check(name, params, cfg, batch, chans, height, width)) return rc;
    SPV_CHECK(spv_loader_augment_supported(chans, height, width),
              "%s: a %d x %d x %d image is not supported (two fp32 copies of the image, the reduction slots and %d bytes of hand-over "
              "within %d bytes of LDS): fetch with mode none, then spv_augment_params and spv_augment_u8 / spv_augment_tiled_u8",
              name, chans, height, width, (int)(FUSED_TAIL_FLOATS * sizeof(float)), AUG_LDS_BYTES);
    SPV_CHECK(((uintptr_t)out_nchw & 3) == 0, "%s: out must be 4-byte aligned", name);
    FusedArgs a;
    a.src = src_nhwc;
    a.labels_src = labels_src;
    a.cursor = static_cast<unsigned long long*>(cursor);
    a.index = index;
    a.labels = labels;
    a.params = params;
    a.out = out_nchw;
    a.mean = mean;
    a.inv_std = inv_std;
    a.loader_seed = loader_seed;
    a.augment_seed = augment_seed;
    a.g = LdrGeom{(uint32_t)n, (uint32_t)batch, (uint32_t)world, (uint32_t)rank, (uint32_t)steps_per_epoch, shuffle != 0};
    a.cfg = *cfg;
    a.H = height;
    a.W = width;
    a.vec = (height * width) % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0;
    a.label_i64 = label_dtype == SPV_LOADER_LABEL_I64;
    const size_t lds = fused_lds_bytes(chans, height, width);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (chans == 3) hipLaunchKernelGGL(loader_augment_kernel<3>, dim3(batch), dim3(AUG_THREADS), lds, st, a);
    else hipLaunchKernelGGL(loader_augment_kernel<1>, dim3(batch), dim3(AUG_THREADS), lds, st, a);
    SPV_LAUNCH_CHECK(name);
    SPV_COUNT_PATH(SPV_PATH_AUGMENT);
    return 0;
}
