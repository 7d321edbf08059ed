// The training transform chain on output TILES, for images the whole-image kernel of spv_augment.hip cannot stage in LDS (64 x 64 up to
// 512 x 512): the same definition, parameter table and random stream (include/spv.h).  Up to the rotation the
// chain is a per-pixel function of (source pixel, parameter row, contrast mean), so a tile evaluates it at the gathered source position;
// the two non-local things are the contrast mean (a pre-pass of per-workgroup partial sums, folded in a fixed order by every tile) and
// the 3 x 3 blur (a one-pixel halo round the tile, in LDS).  At the end of the file the resident loader's fetch, the draw and the
// pre-pass as ONE kernel that reads the step from the loader's device cursor (spv_loader_fetch_augment_tiled).
#include "spv_common.h"
#include "spv_augment_core.h"
#include "spv_augment_draw.h"   // the fused fetch: the draw of a table row and its host checks
#include "spv_loader_core.h"    // the fused fetch: the sample order and the cursor's protocol
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
// ONE definition of a workgroup's partial, for the pre-pass below and for the fused fetch at the end of this file: `p` is the sample's
// table row (global memory there, LDS here), `row` its row of the set, `out` = &ws[b][k], `red` four LDS floats.
template <int C>
__device__ __forceinline__ void aug_mean_part(const unsigned char* __restrict__ src, int64_t row, const float* p, float* __restrict__ out,
                                              float* red, int n_src, int H, int W, int rows, int k) {
    const int tid = threadIdx.x;
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
    if (tid == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

template <int C>
__global__ __launch_bounds__(AUGT_THREADS) void augment_mean_kernel(const unsigned char* __restrict__ src, const int64_t* __restrict__ index,
                                                                    const float* __restrict__ params, float* __restrict__ ws, int n_src,
                                                                    int H, int W, int rows, int parts) {
    __shared__ float red[4];
    const int b = blockIdx.x / parts, k = blockIdx.x - b * parts;
    const int64_t row = index != nullptr ? index[b] : (int64_t)b;
    aug_mean_part<C>(src, row, params + (size_t)b * SPV_AUG_NPARAM, ws + (size_t)b * parts + k, red, n_src, H, W, rows, k);
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

// ---------------------------------------------------------------- host: what both entry points check and launch
static int tiled_check(const char* name, const unsigned char* src_nhwc, const int64_t* index, const float* params, const float* mean,
                       const float* inv_std, const float* out_nchw, int batch, int n_src, int chans, int height, int width,
                       const void* workspace, size_t workspace_bytes) {
    SPV_CHECK(batch > 0 && n_src > 0 && chans > 0 && height > 0 && width > 0, "%s: bad shape", name);
    SPV_CHECK(tiled_takes(chans, height, width), "%s: a %d x %d x %d image is not supported (1 or 3 channels, height and width in [2, %d])",
              name, chans, height, width, AUGT_MAX_SIDE);
    SPV_CHECK(src_nhwc != nullptr && out_nchw != nullptr, "%s: src / out missing", name);
    SPV_CHECK(params != nullptr, "%s: params missing", name);
    SPV_CHECK(mean != nullptr && inv_std != nullptr, "%s: mean / inv_std missing", name);
    SPV_CHECK(index != nullptr || batch <= n_src, "%s: index == NULL reads rows 0..batch-1, but batch=%d > n_src=%d", name, batch, n_src);
    SPV_CHECK(((uintptr_t)out_nchw & 3) == 0 && ((uintptr_t)params & 3) == 0, "%s: out / params must be 4-byte aligned", name);
    const size_t need = spv_augment_tiled_ws_bytes(batch, height, width);
    SPV_CHECK(workspace != nullptr && workspace_bytes >= need,
              "%s: workspace missing or too small (%zu bytes, spv_augment_tiled_ws_bytes asks for %zu)", name,
              workspace == nullptr ? (size_t)0 : workspace_bytes, need);
    SPV_CHECK(((uintptr_t)workspace & 3) == 0, "%s: workspace must be 4-byte aligned", name);
    static_assert(AUGT_MAX_PARTS >= AUGT_MAX_SIDE / (AUGT_MEAN_PIXELS / AUGT_MAX_SIDE), "the fold is at most 64 additions");
    const int64_t tiles = (int64_t)cdiv(width, AUGT_TW) * cdiv(height, AUGT_TH);
    SPV_CHECK((int64_t)batch * tiles <= INT_MAX && (int64_t)batch * mean_parts(height, width) <= INT_MAX, "%s: batch=%d is too large a grid",
              name, batch);
    return 0;
}

static void launch_tiles(const unsigned char* src_nhwc, const int64_t* index, const float* params, const float* mean, const float* inv_std,
                         const float* ws, float* out_nchw, int batch, int n_src, int chans, int height, int width, hipStream_t st) {
    const int parts = mean_parts(height, width);
    const int tiles_x = cdiv(width, AUGT_TW), tiles = tiles_x * cdiv(height, AUGT_TH);
    const int vec = width % 4 == 0 && ((uintptr_t)out_nchw & 15) == 0;
    if (chans == 3)
        hipLaunchKernelGGL(augment_tile_kernel<3>, dim3(batch * tiles), dim3(AUGT_THREADS), 0, st, src_nhwc, index, params, mean, inv_std, ws,
                           out_nchw, n_src, height, width, tiles_x, tiles, parts, vec);
    else
        hipLaunchKernelGGL(augment_tile_kernel<1>, dim3(batch * tiles), dim3(AUGT_THREADS), 0, st, src_nhwc, index, params, mean, inv_std, ws,
                           out_nchw, n_src, height, width, tiles_x, tiles, parts, vec);
}

extern "C" int spv_augment_tiled_u8(const unsigned char* src_nhwc, const int64_t* index, const float* params, const float* mean,
                                    const float* inv_std, float* out_nchw, int batch, int n_src, int chans, int height, int width,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = tiled_check("spv_augment_tiled_u8", src_nhwc, index, params, mean, inv_std, out_nchw, batch, n_src, chans, height, width,
                             workspace, workspace_bytes))
        return rc;
    const int parts = mean_parts(height, width), rows = mean_rows(width);
    float* ws = static_cast<float*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (chans == 3)
        hipLaunchKernelGGL(augment_mean_kernel<3>, dim3(batch * parts), dim3(AUGT_THREADS), 0, st, src_nhwc, index, params, ws, n_src, height,
                           width, rows, parts);
    else
        hipLaunchKernelGGL(augment_mean_kernel<1>, dim3(batch * parts), dim3(AUGT_THREADS), 0, st, src_nhwc, index, params, ws, n_src, height,
                           width, rows, parts);
    launch_tiles(src_nhwc, index, params, mean, inv_std, ws, out_nchw, batch, n_src, chans, height, width, st);
    SPV_LAUNCH_CHECK("spv_augment_tiled_u8");
    SPV_COUNT_PATH(SPV_PATH_AUGMENT);
    return 0;
}

// ---------------------------------------------------------------- fetch, draw and pre-pass in one launch
// spv_loader_fetch(mode none) at the cursor's step t, spv_augment_params(step = t) and the pre-pass above as ONE launch on the
// pre-pass's grid, then the tile kernel unchanged: nothing of either launch is a by-value function of the step, so a captured pair
// draws a new batch AND a new table at every replay.
struct TiledFetchArgs {
    const unsigned char* src;     // [n][H][W][C]
    const void* labels_src;       // [n] uint8 or int64
    unsigned long long* cursor;   // the loader's cursor block
    int64_t* index;               // [batch]
    int64_t* labels;              // [batch]
    float* params;                // [batch][16]
    float* ws;                    // [batch][parts]
    uint64_t loader_seed, augment_seed;
    LdrGeom g;
    spv_augment_cfg cfg;
    int H, W, rows, parts, label_i64;
};

// Workgroup (image b, chunk k).  Thread 0 reads the step and hands it round; the sample's row of the set (wave 0) and its table row
// (wave 1) -- functions of (t, b) alone, so all `parts` workgroups of an image work out the same two -- go round through LDS, never
// through `index` / `params` in global memory: what a sibling workgroup writes there is not visible inside the launch.  Chunk 0 records
// them for the tile kernel and the caller.  Wave 2 takes the ticket behind the read of t (it came through LDS and two barriers, so the
// load has returned: no fence); EVERY workgroup takes one, also the one whose contrast factor is 1 and whose partial nobody reads --
// the early return sits inside aug_mean_part, behind the ticket.
template <int C>
__global__ __launch_bounds__(AUGT_THREADS) void loader_mean_kernel(TiledFetchArgs a) {
    __shared__ __attribute__((aligned(16))) float row_sh[SPV_AUG_NPARAM];
    __shared__ unsigned long long t_sh;
    __shared__ uint32_t idx_sh;
    __shared__ float red[4];
    const uint32_t b = blockIdx.x / (uint32_t)a.parts;
    const int k = (int)(blockIdx.x - b * (uint32_t)a.parts), tid = threadIdx.x;
    if (tid == 0) t_sh = ldr_read_step(a.cursor);
    __syncthreads();
    const uint64_t t = t_sh;
    if (tid == 0) {
        const uint32_t idx = ldr_index(a.loader_seed, t, b, a.g);   // < n by construction (spv_loader_core.h)
        if (k == 0) {
            a.index[b] = (int64_t)idx;
            a.labels[b] = a.label_i64 ? static_cast<const int64_t*>(a.labels_src)[idx]
                                      : (int64_t) static_cast<const unsigned char*>(a.labels_src)[idx];
        }
        idx_sh = idx;
    } else if (tid == 64) {
        const AugRow r = aug_draw(a.H, a.W, a.cfg, a.augment_seed, t, b);
        if (k == 0) aug_store_row(a.params, b, r);
#pragma unroll
        for (int i = 0; i < SPV_AUG_NPARAM; ++i) row_sh[i] = r.v[i];
    }
    __syncthreads();
    if (tid == 128) ldr_arrive<false>(a.cursor, t, a.g.batch * (unsigned)a.parts);   // groups = batch * parts: the whole grid
    aug_mean_part<C>(a.src, (int64_t)idx_sh, row_sh, a.ws + (size_t)b * a.parts + k, red, (int)a.g.n, a.H, a.W, a.rows, k);
}

extern "C" int spv_loader_augment_tiled_supported(int chans, int height, int width) { return tiled_takes(chans, height, width) ? 1 : 0; }

extern "C" int spv_loader_fetch_augment_tiled(const unsigned char* src_nhwc, const void* labels_src, void* cursor, int64_t* index,
                                              int64_t* labels, float* params, float* out_nchw, const float* mean, const float* inv_std,
                                              const spv_augment_cfg* cfg, int n, int batch, int chans, int height, int width, int world,
                                              int rank, int steps_per_epoch, uint64_t loader_seed, int shuffle, int label_dtype,
                                              uint64_t augment_seed, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "spv_loader_fetch_augment_tiled";
    // the fetch's refusals (as its float mode: src, img, mean and inv_std are all read), then the draw's, then the tiled apply's
    if (int rc = spv_loader_check(name, src_nhwc, labels_src, cursor, index, labels, out_nchw, mean, inv_std, n, batch, chans, height, width,
                                  world, rank, steps_per_epoch, SPV_LOADER_FLOAT, label_dtype))
        return rc;
    if (int rc = aug_draw_check(name, params, cfg, batch, chans, height, width)) return rc;
    if (int rc = tiled_check(name, src_nhwc, index, params, mean, inv_std, out_nchw, batch, n, chans, height, width, workspace, workspace_bytes))
        return rc;
    TiledFetchArgs a;
    a.src = src_nhwc;
    a.labels_src = labels_src;
    a.cursor = static_cast<unsigned long long*>(cursor);
    a.index = index;
    a.labels = labels;
    a.params = params;
    a.ws = static_cast<float*>(workspace);
    a.loader_seed = loader_seed;
    a.augment_seed = augment_seed;
    a.g = LdrGeom{(uint32_t)n, (uint32_t)batch, (uint32_t)world, (uint32_t)rank, (uint32_t)steps_per_epoch, shuffle != 0};
    a.cfg = *cfg;
    a.H = height;
    a.W = width;
    a.rows = mean_rows(width);
    a.parts = mean_parts(height, width);
    a.label_i64 = label_dtype == SPV_LOADER_LABEL_I64;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (chans == 3) hipLaunchKernelGGL(loader_mean_kernel<3>, dim3(batch * a.parts), dim3(AUGT_THREADS), 0, st, a);
    else hipLaunchKernelGGL(loader_mean_kernel<1>, dim3(batch * a.parts), dim3(AUGT_THREADS), 0, st, a);
    launch_tiles(src_nhwc, index, params, mean, inv_std, a.ws, out_nchw, batch, n, chans, height, width, st);
    SPV_LAUNCH_CHECK(name);
    SPV_COUNT_PATH(SPV_PATH_AUGMENT);
    return 0;
}

