// The draw of the training transform's parameter table (include/spv.h): ONE definition of a sample's sixteen
// numbers and of the host checks of every entry point that draws them -- the table kernel and the fused fetch of spv_augment.hip, the
// fused tiled fetch of spv_augment_tiled.hip.  Needs spv_common.h (mix32, SPV_CHECK) in front of it.
#pragma once
#include "spv_common.h"
#include <math.h>

// ---------------------------------------------------------------- parameter draws
// uniform in [0, 1) with 24 bits, draw `d` of the sample whose key is `key`
__device__ __forceinline__ float aug_u01(unsigned key, unsigned d) {
    return (float)(mix32(key + (d + 1u) * 0xc2b2ae35u) >> 8) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float aug_range(float lo, float hi, float u) { return lo + (hi - lo) * u; }

// the sixteen numbers of one sample: the table row
struct AugRow {
    float v[SPV_AUG_NPARAM];
};

// sample slot `s` of `step`: ONE definition of the draw, for the table kernel and for the fused fetches
__device__ __forceinline__ AugRow aug_draw(int H, int W, const spv_augment_cfg& c, uint64_t seed, uint64_t step, unsigned s) {
    unsigned key = mix32((unsigned)seed + 0x9e3779b1u) ^ mix32((unsigned)(seed >> 32) + 0x7f4a7c15u);
    key = mix32(key + (unsigned)step * 0x85ebca6bu) ^ mix32((unsigned)(step >> 32) + 0x27d4eb2fu);
    key = mix32(key + s * 0x9e3779b1u);
    AugRow row;
    float* p = row.v;
#pragma unroll
    for (int i = 0; i < SPV_AUG_NPARAM; ++i) p[i] = 0.0f;
    p[SPV_AUG_FLIP] = aug_u01(key, 0) < c.flip_p ? 1.0f : 0.0f;
    p[SPV_AUG_BRIGHT] = aug_range(c.bright_lo, c.bright_hi, aug_u01(key, 1));
    p[SPV_AUG_CONTRAST] = aug_range(c.contrast_lo, c.contrast_hi, aug_u01(key, 2));
    p[SPV_AUG_SAT] = aug_range(c.sat_lo, c.sat_hi, aug_u01(key, 3));
    p[SPV_AUG_HUE] = aug_range(c.hue_lo, c.hue_hi, aug_u01(key, 4));
    p[SPV_AUG_ORDER] = (float)min((int)(aug_u01(key, 5) * 24.0f), 23);
    p[SPV_AUG_GRAY] = aug_u01(key, 6) < c.gray_p ? 1.0f : 0.0f;
    p[SPV_AUG_ANGLE] = aug_range(-c.degrees, c.degrees, aug_u01(key, 7));
    p[SPV_AUG_BLUR] = aug_u01(key, 8) < c.blur_p ? 1.0f : 0.0f;
    p[SPV_AUG_SIGMA] = aug_range(c.sigma_lo, c.sigma_hi, aug_u01(key, 9));
    if (aug_u01(key, 10) < c.erase_p) {
        // RandomErasing.get_params: up to ten attempts, the first rectangle that fits wins
        const float area = (float)(H * W), llo = logf(c.ratio_lo), lhi = logf(c.ratio_hi);
        for (int a = 0; a < 10; ++a) {
            const unsigned d = 11u + 4u * (unsigned)a;
            const float ea = area * aug_range(c.scale_lo, c.scale_hi, aug_u01(key, d));
            const float ratio = expf(aug_range(llo, lhi, aug_u01(key, d + 1)));
            const int h = (int)rintf(sqrtf(ea * ratio)), w = (int)rintf(sqrtf(ea / ratio));
            if (!(h < H && w < W)) continue;
            p[SPV_AUG_ERASE_I] = (float)min((int)(aug_u01(key, d + 2) * (float)(H - h + 1)), H - h);
            p[SPV_AUG_ERASE_J] = (float)min((int)(aug_u01(key, d + 3) * (float)(W - w + 1)), W - w);
            p[SPV_AUG_ERASE_H] = (float)h;
            p[SPV_AUG_ERASE_W] = (float)w;
            break;
        }
    }
    return row;
}
// the row to the table (params 16-byte aligned: four 16-byte stores)
__device__ __forceinline__ void aug_store_row(float* params, unsigned s, const AugRow& row) {
    float4* o = reinterpret_cast<float4*>(params + (size_t)s * SPV_AUG_NPARAM);
#pragma unroll
    for (int i = 0; i < SPV_AUG_NPARAM / 4; ++i) o[i] = make_float4(row.v[4 * i], row.v[4 * i + 1], row.v[4 * i + 2], row.v[4 * i + 3]);
}

// the checks of every entry point that draws a table (spv_augment_params, spv_loader_fetch_augment, spv_loader_fetch_augment_tiled): on
// the host, before any launch
static inline int aug_draw_check(const char* name, const float* params, const spv_augment_cfg* cfg, int batch, int chans, int height,
                                 int width) {
    SPV_CHECK(params != nullptr && cfg != nullptr, "%s: params / cfg missing", name);
    SPV_CHECK(((uintptr_t)params & 15) == 0, "%s: params must be 16-byte aligned", name);
    SPV_CHECK(batch > 0 && (chans == 1 || chans == 3) && height >= 2 && width >= 2 && height <= 4096 && width <= 4096,
              "%s: bad shape batch=%d chans=%d %dx%d", name, batch, chans, height, width);
    const spv_augment_cfg& c = *cfg;
    const bool probs = c.flip_p >= 0.0f && c.flip_p <= 1.0f && c.gray_p >= 0.0f && c.gray_p <= 1.0f && c.blur_p >= 0.0f &&
                       c.blur_p <= 1.0f && c.erase_p >= 0.0f && c.erase_p <= 1.0f;
    SPV_CHECK(probs, "%s: a probability outside [0, 1]", name);
    const bool ranges = c.bright_lo >= 0.0f && c.bright_lo <= c.bright_hi && c.contrast_lo >= 0.0f && c.contrast_lo <= c.contrast_hi &&
                        c.sat_lo >= 0.0f && c.sat_lo <= c.sat_hi && c.hue_lo >= -0.5f && c.hue_lo <= c.hue_hi && c.hue_hi <= 0.5f &&
                        c.degrees >= 0.0f && c.degrees <= 180.0f && c.sigma_lo > 0.0f && c.sigma_lo <= c.sigma_hi && c.scale_lo >= 0.0f &&
                        c.scale_lo <= c.scale_hi && c.scale_hi <= 1.0f && c.ratio_lo > 0.0f && c.ratio_lo <= c.ratio_hi;
    SPV_CHECK(ranges, "%s: a range is empty or outside its op's domain", name);
    return 0;
}
