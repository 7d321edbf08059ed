// The per-pixel part of the training transform chain (include/spv.h): ONE body for the contrast mean's pre-pass
// and the tile kernel of spv_augment_tiled.hip, whose pixels must see the same ops in the same order, and the helpers of the whole-image
// kernel of spv_augment.hip.  Host/device, no HIP type in it: tests/test_augment_tiled.py compiles it with a plain C++ compiler and
// holds the chain of all 24 orders to tests/augment_ref.py.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SPV_AUG_HD __host__ __device__ __forceinline__
#else
#define SPV_AUG_HD inline
#endif

// the four ColorJitter ops as the order index counts them (lexicographic over b, c, s, h)
constexpr int AUG_OP_BRIGHT = 0, AUG_OP_CONTRAST = 1, AUG_OP_SAT = 2, AUG_OP_HUE = 3, AUG_OP_NONE = 4;

SPV_AUG_HD float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
SPV_AUG_HD float grey_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// torchvision's _rgb2hsv / _hsv2rgb (the hexcone formulas) with h := frac(h + shift) between them
SPV_AUG_HD void hue_shift(float& r, float& g, float& b, float shift) {
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
    const float d = mx - mn;
    const bool flat = d == 0.0f;
    const float v = mx;
    const float s = flat ? 0.0f : d / mx;
    const float dd = flat ? 1.0f : d;
    const float rc = (mx - r) / dd, gc = (mx - g) / dd, bc = (mx - b) / dd;
    const float h6 = mx == r ? bc - gc : (mx == g ? 2.0f + rc - bc : 4.0f + gc - rc);
    float h = h6 / 6.0f + 1.0f;
    h -= floorf(h);
    h += shift;
    h -= floorf(h);
    const float h6b = h * 6.0f;
    const float fi = floorf(h6b);
    const float f = h6b - fi;
    int i = (int)fi % 6;
    const float p = clamp01(v * (1.0f - s));
    const float q = clamp01(v * (1.0f - s * f));
    const float t = clamp01(v * (1.0f - s * (1.0f - f)));
    r = i == 0 ? v : (i == 1 ? q : (i == 2 ? p : (i == 3 ? p : (i == 4 ? t : v))));
    g = i == 0 ? t : (i == 1 ? v : (i == 2 ? v : (i == 3 ? q : (i == 4 ? p : p))));
    b = i == 0 ? p : (i == 1 ? p : (i == 2 ? t : (i == 3 ? v : (i == 4 ? v : q))));
}

// the order index of a parameter row, clamped to the 24 permutations
SPV_AUG_HD int aug_order_index(float order) {
    const int idx = (int)order;
    return idx < 0 ? 0 : (idx > 23 ? 23 : idx);
}

// op number k (0..3) of permutation `idx`; `avail` holds the ops not yet used, one per nibble, ascending (0x3210 in front of k = 0)
SPV_AUG_HD int aug_order_next(int idx, int k, unsigned& avail) {
    const int n = k == 0 ? idx / 6 : (k == 1 ? (idx % 6) / 2 : (k == 2 ? idx % 2 : 0));
    const int op = (int)((avail >> (4 * n)) & 0xfu);
    avail = (avail & ((1u << (4 * n)) - 1u)) | ((avail >> (4 * n + 4)) << (4 * n));
    return op;
}

struct AugJitter {
    float bright, contrast, sat, hue;   // SPV_AUG_BRIGHT .. SPV_AUG_HUE of the sample's row
    int order;                          // aug_order_index(SPV_AUG_ORDER)
};

// The jitter ops of order j.order on one pixel v (C = 1: v[0] only; saturation and hue are the identity), up to but NOT including the
// first op equal to `stop` (AUG_OP_NONE: all four).  m = the image's contrast mean, read only when contrast is among the ops run.
template <int C>
SPV_AUG_HD void aug_jitter_pixel(float (&v)[3], const AugJitter& j, float m, int stop) {
    unsigned avail = 0x3210u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const int op = aug_order_next(j.order, k, avail);
        if (op == stop) return;
        if (op == AUG_OP_BRIGHT) {
            for (int c = 0; c < C; ++c) v[c] = clamp01(v[c] * j.bright);
        } else if (op == AUG_OP_CONTRAST) {
            const float add = (1.0f - j.contrast) * m;
            for (int c = 0; c < C; ++c) v[c] = clamp01(j.contrast * v[c] + add);
        } else if (op == AUG_OP_SAT) {
            if (C == 3) {
                const float gr = (1.0f - j.sat) * grey_of(v[0], v[1], v[2]);
                for (int c = 0; c < 3; ++c) v[c] = clamp01(j.sat * v[c] + gr);
            }
        } else {
            if (C == 3 && j.hue != 0.0f) hue_shift(v[0], v[1], v[2], j.hue);
        }
    }
}

// what the contrast mean averages: the pixel's grey value after the ops in front of contrast
template <int C>
SPV_AUG_HD float aug_grey_before_contrast(float (&v)[3], const AugJitter& j) {
    aug_jitter_pixel<C>(v, j, 0.0f, AUG_OP_CONTRAST);
    return C == 3 ? grey_of(v[0], v[1], v[2]) : v[0];
}

// the whole per-pixel chain in front of the rotation: jitter in the drawn order, then RandomGrayscale
template <int C>
SPV_AUG_HD void aug_colour_pixel(float (&v)[3], const AugJitter& j, float m, bool gray) {
    aug_jitter_pixel<C>(v, j, m, AUG_OP_NONE);
    if (C == 3 && gray) {
        const float gr = grey_of(v[0], v[1], v[2]);
        v[0] = gr;
        v[1] = gr;
        v[2] = gr;
    }
}

// RandomAffine(degrees)'s inverse map as torchvision hands it to PIL: source = (cs X + sn Y + tx, -sn X + cs Y + ty), X, Y pixel centres
struct AugRotation {
    float cs, sn, tx, ty;
};
SPV_AUG_HD AugRotation aug_rotation(float angle_degrees, int H, int W) {
    const float rad = -angle_degrees * 0.017453292519943295f;
    AugRotation r;
    r.cs = cosf(rad);
    r.sn = sinf(rad);
    const float cx = 0.5f * (float)W, cy = 0.5f * (float)H;
    r.tx = cx - cx * r.cs - cy * r.sn;
    r.ty = cy + cx * r.sn - cy * r.cs;
    return r;
}
// nearest-neighbour source pixel of output pixel (y, x); false = outside the image (zero fill)
SPV_AUG_HD bool aug_rotation_source(const AugRotation& r, int y, int x, int H, int W, int& iy, int& ix) {
    const float X = (float)x + 0.5f, Y = (float)y + 0.5f;
    const float sx = r.cs * X + r.sn * Y + r.tx, sy = -r.sn * X + r.cs * Y + r.ty;
    ix = (int)floorf(sx);
    iy = (int)floorf(sy);
    return ix >= 0 && ix < W && iy >= 0 && iy < H;
}
