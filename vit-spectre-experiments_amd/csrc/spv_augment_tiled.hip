// The training transform chain on output TILES, for images the whole-image kernel of spv_augment.hip cannot stage in LDS (64 x 64 up to
// 512 x 512): the same definition, parameter table and random stream (include/spv.h).  Up to the rotation the
// chain is a per-pixel function of (source pixel, parameter row, contrast mean), so a tile evaluates it at the gathered source position;
// the two non-local things are the contrast mean (a pre-pass of per-workgroup partial sums, folded in a fixed order by every tile) and
// the 3 x 3 blur (a one-pixel halo round the tile, in LDS).
#include "spv_common.h"
#include "spv_augment_core.h"
#include <limits.h>

constexpr int AUGT_THREADS = 256;
constexpr int AUGT_TH = 16, AUGT_TW = 64;                 // output tile: 16 rows of 64 pixels, 4 pixels per thread
constexpr int AUGT_HH = AUGT_TH + 2, AUGT_HW = AUGT_TW + 2;   // with the blur's halo
constexpr int AUGT_QUADS = AUGT_TH * AUGT_TW / 4;
static_assert(AUGT_QUADS == AUGT_THREADS, "one quad of four pixels per thread");
constexpr int AUGT_MEAN_PIXELS = 4096;                    // pixels per pre-pass workgroup: 16 per thread
constexpr int AUGT_MAX_SIDE = 512;
constexpr int AUGT_MAX_PARTS = 64;                        // mean_parts(512, 512)

// rows per pre-pass workgroup and partial sums per image
static inline int mean_rows(int width) { return AUGT_MEAN_PIXELS / width > 0 ? AUGT_MEAN_PIXELS / width : 1; }
static inline int mean_parts(int height, int width) { return cdiv(height, mean_rows(width)); }

extern "C" int spv_augment_plan(int chans, int height, int width) {
    if (spv_augment_supported(chans, height, width)) return 1;
    if (!(chans == 1 || chans == 3) || height < 2 || width < 2 || height > AUGT_MAX_SIDE || width > AUGT_MAX_SIDE) return 0;
    return 2;
}

static inline bool tiled_takes(int chans, int height, int width) {
    return (chans == 1 || chans == 3) && height >= 2 && width >= 2 && height <= AUGT_MAX_SIDE && width <= AUGT_MAX_SIDE;
}

extern "C" size_t spv_augment_tiled_ws_bytes(int batch, int height, int width) {
    if (batch <= 0 || height < 2 || width < 2 || height > AUGT_MAX_SIDE || width > AUGT_MAX_SIDE) return 0;
    return (size_t)batch * mean_parts(height, width) * sizeof(float);
}

struct AugSample {
    AugJitter j;
    bool flip, gray;
};
__device__ __forceinline__ AugSample aug_sample(const float* __restrict__ p) {
    AugSample s;
    s.j.bright = p[SPV_AUG_BRIGHT];
    s.j.contrast = p[SPV_AUG_CONTRAST];
    s.j.sat = p[SPV_AUG_SAT];
    s.j.hue = p[SPV_AUG_HUE];
    s.j.order = aug_order_index(p[SPV_AUG_ORDER]);
    s.flip = p[SPV_AUG_FLIP] != 0.0f;
    s.gray = p[SPV_AUG_GRAY] != 0.0f;
    return s;
}

template <int C>
__device__ __forceinline__ void load_pixel(const unsigned char* __restrict__ img, int pos, float (&v)[3]) {
    const unsigned char* s = img + (size_t)pos * C;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (float)s[c] / 255.0f;
}

// ---------------------------------------------------------------- the contrast mean's partial sums
// Workgroup (image b, chunk k) sums the grey values (after the ops in front of contrast) of rows [k rows, (k + 1) rows) and writes
// ws[b][k].  A flip permutes a row and is left out.  fp32 only over a thread's <= 16 pixels, a wave, the four waves; no atomics.
template <int C>
__global__ __launch_bounds__(AUGT_THREADS) void augment_mean_kernel(const unsigned char* __restrict__ src, const int64_t* __restrict__ index,
                                                                    const float* __restrict__ params, float* __restrict__ ws, int n_src,
                                                                    int H, int W, int rows, int parts) {
    __shared__ float red[4];
    const int b = blockIdx.x / parts, k = blockIdx.x - b * parts, tid = threadIdx.x;
    const float* p = params + (size_t)b * SPV_AUG_NPARAM;
    const int64_t row = index != nullptr ? index[b] : (int64_t)b;
    // workgroup uniform: f x + (1 - f) m is x at f == 1, and a poisoned image reads nothing; the tile kernel skips the fold alike
    if (p[SPV_AUG_CONTRAST] == 1.0f || row < 0 || row >= (int64_t)n_src) return;
    const AugSample s = aug_sample(p);
    const unsigned char* img = src + (size_t)row * H * W * C;
    const int first = k * rows * W, last = min((k + 1) * rows, H) * W;
    float part = 0.0f;
    for (int px = first + tid; px < last; px += AUGT_THREADS) {
        float v[3];
        load_pixel<C>(img, px, v);
        part += aug_grey_before_contrast<C>(v, s.j);
    }
    part = wave_sum(part);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) ws[(size_t)b * parts + k] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------- the tile kernel
struct AugTileCtx {
    AugSample s;
    AugRotation rot;
    bool rotate;
    float m;
    int H, W;
};

// rotated, jittered, grey-scaled pixel (y, x) of the image in front of the blur: the flip comes first in the chain, so rotated pixel
// (iy, ix) reads raw (iy, W - 1 - ix)
template <int C>
__device__ __forceinline__ void chain_pixel(const unsigned char* __restrict__ img, const AugTileCtx& t, int y, int x, float (&v)[3]) {
    int iy = y, ix = x;
    const bool in = t.rotate ? aug_rotation_source(t.rot, y, x, t.H, t.W, iy, ix) : true;
    if (!in) {
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0.0f;
        return;
    }
    load_pixel<C>(img, iy * t.W + (t.s.flip ? t.W - 1 - ix : ix), v);
    aug_colour_pixel<C>(v, t.s.j, t.m, t.s.gray);
}

// LDS of a blurring tile: `a` [C][18][66] the chain's pixels of tile + halo (local (ly, lx) = image (y0 - 1 + ly, x0 - 1 + lx)), `h`
// [C][18][64] their horizontal pass over the tile's columns.  Every pass walks a row with consecutive lanes: the fill writes flat
// consecutive dwords, the horizontal pass reads three and writes one consecutive run per 64-lane row (ds_read_b32 / ds_write_b32 bank =
// dword % 32, a 32-lane group covers 32 consecutive dwords), and the vertical pass reads float4 at a 256-byte row pitch, lane l at
// 16-byte slot l of its group (ds_read_b128, bank = dword % 64: 16 lanes cover one bank row): no conflict in any of them, whatever the
// pitch, because no pass walks a column.
template <int C>
__global__ __launch_bounds__(AUGT_THREADS) void augment_tile_kernel(const unsigned char* __restrict__ src, const int64_t* __restrict__ index,
                                                                    const float* __restrict__ params, const float* __restrict__ mean,
                                                                    const float* __restrict__ inv_std, const float* __restrict__ ws,
                                                                    float* __restrict__ out, int n_src, int H, int W, int tiles_x,
                                                                    int tiles, int parts, int vec) {
    __shared__ __attribute__((aligned(16))) float a[C * AUGT_HH * AUGT_HW];
    __shared__ __attribute__((aligned(16))) float h[C * AUGT_HH * AUGT_TW];
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles, tid = threadIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * AUGT_TH, x0 = tx * AUGT_TW;
    const int HW = H * W;
    const float* p = params + (size_t)b * SPV_AUG_NPARAM;
    float* o = out + (size_t)b * C * HW;
    // this thread's quad: row qy, columns qx .. qx + 3 of the image
    const int qy = y0 + tid / (AUGT_TW / 4), qx = x0 + 4 * (tid % (AUGT_TW / 4));
    const bool quad_in = qy < H && qx < W;
    const bool quad_vec = vec && qx + 3 < W;
    const int64_t row = index != nullptr ? index[b] : (int64_t)b;
    if (row < 0 || row >= (int64_t)n_src) {   // workgroup uniform: nothing is read, the image's tiles are poisoned
        if (quad_in) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                for (int u = 0; u < 4 && qx + u < W; ++u) o[c * HW + qy * W + qx + u] = __builtin_nanf("");
        }
        return;
    }
    const unsigned char* img = src + (size_t)row * HW * C;

    AugTileCtx t;
    t.s = aug_sample(p);
    t.H = H;
    t.W = W;
    const float angle = p[SPV_AUG_ANGLE];
    t.rotate = angle != 0.0f;
    t.rot = aug_rotation(angle, H, W);
    // every workgroup of the image folds the same partials in the same order: one value of m, bit for bit, in all its tiles
    t.m = 0.0f;
    if (t.s.j.contrast != 1.0f) {
        double sum = 0.0;
        for (int k = 0; k < parts; ++k) sum += (double)ws[(size_t)b * parts + k];
        t.m = (float)(sum / (double)HW);
    }

    float r[C][4];
    if (p[SPV_AUG_BLUR] == 0.0f) {   // workgroup uniform: no neighbour is read, no LDS
        if (quad_in) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float v[3] = {0.0f, 0.0f, 0.0f};
                if (qx + u < W) chain_pixel<C>(img, t, qy, qx + u, v);
#pragma unroll
                for (int c = 0; c < C; ++c) r[c][u] = v[c];
            }
        }
    } else {
        const float sigma = p[SPV_AUG_SIGMA];
        const float e = expf(-1.0f / (2.0f * sigma * sigma));
        const float norm = 1.0f + 2.0f * e;
        const float w0 = 1.0f / norm, w1 = e / norm;
        // tile + halo; what lies outside the image is never read (the reflection stays inside, see below) and is written zero
        for (int i = tid; i < AUGT_HH * AUGT_HW; i += AUGT_THREADS) {
            const int ly = i / AUGT_HW, lx = i - ly * AUGT_HW;
            const int y = y0 - 1 + ly, x = x0 - 1 + lx;
            float v[3] = {0.0f, 0.0f, 0.0f};
            if (y >= 0 && y < H && x >= 0 && x < W) chain_pixel<C>(img, t, y, x, v);
#pragma unroll
            for (int c = 0; c < C; ++c) a[c * AUGT_HH * AUGT_HW + i] = v[c];
        }
        __syncthreads();
        // horizontal pass over the tile's columns of tile + halo rows.  Reflect padding -1 -> 1, W -> W - 2: column 1 lies in the first
        // tile (W >= 2) and column W - 2 is the last tile's own or, when that tile is one column wide, its halo column.
        for (int i = tid; i < AUGT_HH * AUGT_TW; i += AUGT_THREADS) {
            const int ly = i / AUGT_TW, lc = i - ly * AUGT_TW;
            const int y = y0 - 1 + ly, x = x0 + lc;
            if (y < 0 || y >= H || x >= W) continue;
            const int xl = (x == 0 ? 1 : x - 1) - (x0 - 1), xr = (x == W - 1 ? W - 2 : x + 1) - (x0 - 1);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float* ar = a + c * AUGT_HH * AUGT_HW + ly * AUGT_HW;
                h[c * AUGT_HH * AUGT_TW + i] = w1 * ar[xl] + w0 * ar[lc + 1] + w1 * ar[xr];
            }
        }
        __syncthreads();
        // vertical pass over the tile: rows 1 and H - 2 of the reflection likewise lie in the tile or are its halo row (H = 16 k + 1)
        if (quad_in) {
            const int yu = (qy == 0 ? 1 : qy - 1) - (y0 - 1), yd = (qy == H - 1 ? H - 2 : qy + 1) - (y0 - 1), yc = qy - (y0 - 1);
            const int lc = qx - x0;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float* hp = h + c * AUGT_HH * AUGT_TW + lc;
                const float4 up = *reinterpret_cast<const float4*>(hp + yu * AUGT_TW);
                const float4 ce = *reinterpret_cast<const float4*>(hp + yc * AUGT_TW);
                const float4 dn = *reinterpret_cast<const float4*>(hp + yd * AUGT_TW);
                r[c][0] = w1 * up.x + w0 * ce.x + w1 * dn.x;
                r[c][1] = w1 * up.y + w0 * ce.y + w1 * dn.y;
                r[c][2] = w1 * up.z + w0 * ce.z + w1 * dn.z;
                r[c][3] = w1 * up.w + w0 * ce.w + w1 * dn.w;
            }
        }
    }
    if (!quad_in) return;

    // normalise, erase, store NCHW: a quad leaves as one 16-byte store where W % 4 == 0 and the output is 16-byte aligned
    const int ei = (int)p[SPV_AUG_ERASE_I], ej = (int)p[SPV_AUG_ERASE_J];
    const int eh = (int)p[SPV_AUG_ERASE_H], ew = (int)p[SPV_AUG_ERASE_W];
    const bool row_erased = qy >= ei && qy < ei + eh;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float mu = mean[c], is = inv_std[c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool erased = row_erased && qx + u >= ej && qx + u < ej + ew;
            r[c][u] = erased ? 0.0f : (r[c][u] - mu) * is;
        }
        float* q = o + c * HW + qy * W + qx;
        if (quad_vec) {
            *reinterpret_cast<float4*>(q) = make_float4(r[c][0], r[c][1], r[c][2], r[c][3]);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (qx + u < W) q[u] = r[c][u];
        }
    }
}

extern "C" int spv_augment_tiled_u8(const unsigned char* src_nhwc, const int64_t* index, const float* params, const float* mean,
                                    const float* inv_std, float* out_nchw, int batch, int n_src, int chans, int height, int width,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    SPV_CHECK(batch > 0 && n_src > 0 && chans > 0 && height > 0 && width > 0, "spv_augment_tiled_u8: bad shape");
    SPV_CHECK(tiled_takes(chans, height, width),
              "spv_augment_tiled_u8: a %d x %d x %d image is not supported (1 or 3 channels, height and width in [2, %d])", chans, height,
              width, AUGT_MAX_SIDE);
    SPV_CHECK(src_nhwc != nullptr && out_nchw != nullptr, "spv_augment_tiled_u8: src / out missing");
    SPV_CHECK(params != nullptr, "spv_augment_tiled_u8: params missing");
    SPV_CHECK(mean != nullptr && inv_std != nullptr, "spv_augment_tiled_u8: mean / inv_std missing");
    SPV_CHECK(index != nullptr || batch <= n_src, "spv_augment_tiled_u8: index == NULL reads rows 0..batch-1, but batch=%d > n_src=%d", batch,
              n_src);
    SPV_CHECK(((uintptr_t)out_nchw & 3) == 0 && ((uintptr_t)params & 3) == 0, "spv_augment_tiled_u8: out / params must be 4-byte aligned");
    const size_t need = spv_augment_tiled_ws_bytes(batch, height, width);
    SPV_CHECK(workspace != nullptr && workspace_bytes >= need,
              "spv_augment_tiled_u8: workspace missing or too small (%zu bytes, spv_augment_tiled_ws_bytes asks for %zu)",
              workspace == nullptr ? (size_t)0 : workspace_bytes, need);
    SPV_CHECK(((uintptr_t)workspace & 3) == 0, "spv_augment_tiled_u8: workspace must be 4-byte aligned");
    const int parts = mean_parts(height, width), rows = mean_rows(width);
    const int tiles_x = cdiv(width, AUGT_TW), tiles = tiles_x * cdiv(height, AUGT_TH);
    static_assert(AUGT_MAX_PARTS >= AUGT_MAX_SIDE / (AUGT_MEAN_PIXELS / AUGT_MAX_SIDE), "the fold is at most 64 additions");
    SPV_CHECK((int64_t)batch * tiles <= INT_MAX && (int64_t)batch * parts <= INT_MAX, "spv_augment_tiled_u8: batch=%d is too large a grid",
              batch);
    const int vec = width % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0;
    float* ws = static_cast<float*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (chans == 3) {
        hipLaunchKernelGGL(augment_mean_kernel<3>, dim3(batch * parts), dim3(AUGT_THREADS), 0, st, src_nhwc, index, params, ws, n_src, height,
                           width, rows, parts);
        hipLaunchKernelGGL(augment_tile_kernel<3>, dim3(batch * tiles), dim3(AUGT_THREADS), 0, st, src_nhwc, index, params, mean, inv_std, ws,
                           out_nchw, n_src, height, width, tiles_x, tiles, parts, vec);
    } else {
        hipLaunchKernelGGL(augment_mean_kernel<1>, dim3(batch * parts), dim3(AUGT_THREADS), 0, st, src_nhwc, index, params, ws, n_src, height,
                           width, rows, parts);
        hipLaunchKernelGGL(augment_tile_kernel<1>, dim3(batch * tiles), dim3(AUGT_THREADS), 0, st, src_nhwc, index, params, mean, inv_std, ws,
                           out_nchw, n_src, height, width, tiles_x, tiles, parts, vec);
    }
    SPV_LAUNCH_CHECK("spv_augment_tiled_u8");
    SPV_COUNT_PATH(SPV_PATH_AUGMENT);
    return 0;
}
