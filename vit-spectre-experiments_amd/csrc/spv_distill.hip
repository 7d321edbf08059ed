// Paired-view distillation on the device (reference spectre_vit/repl/train.py:92-100, 139-141, 298-361): the teacher's view of a
// sample -- Resize(resize, BICUBIC) -> CenterCrop(crop) -> ToTensor -> Normalize of the raw 8-bit image, Pillow's integer resampling
// bit for bit -- and the soft-target + cross-entropy loss as one kernel each way.  Definitions: include/spv.h and DESIGN.md section 4d.
#include "spv_common.h"
#include <algorithm>
#include <math.h>

namespace {

// ================================================================ teacher view
constexpr int TV_THREADS = 256;
constexpr int TV_BAND = 32;                // output rows per workgroup: 7 bands at crop 224
constexpr int TV_TAPS = 4;                 // bicubic support 2 without widening (n <= resize)
constexpr int TV_PREC = 22;                // Pillow's PRECISION_BITS for 8-bit images: 32 - 8 - 2
constexpr int TV_LDS_BYTES = 64 * 1024;    // what a workgroup may take without an opt-in attribute
constexpr int TV_MAX_SIDE = 4096;

struct TvPlan {
    int ok, crop_p, max_rows;
    size_t src_bytes, lds;
};

// Pillow's window of output coordinate xx (precompute_coeffs): [xmin, xmax) in source pixels
static inline void tv_window(int xx, int n, int resize, int* xmin, int* xmax) {
    const double scale = (double)n / (double)resize;
    const double center = ((double)xx + 0.5) * scale;
    int lo = (int)(center - 2.0 + 0.5), hi = (int)(center + 2.0 + 0.5);
    *xmin = lo < 0 ? 0 : lo;
    *xmax = hi > n ? n : hi;
}

// The staging plan of one (chans, n, resize, crop): every cropped output must have its four taps inside the image; a band of TV_BAND
// output rows needs the source rows [ymin(first), ymin(last) + 4), at most max_rows of them.  LDS: the coefficient table
// [5][crop_p] int32, the normalisation table [chans][256] fp32, max_rows source rows as they lie (NHWC bytes), and the horizontal
// pass's result [chans][max_rows][crop_p] uint8.
static TvPlan tv_plan(int chans, int n, int resize, int crop) {
    TvPlan p = {0, 0, 0, 0, 0};
    if (!(chans == 1 || chans == 3) || n < 2 || n > resize || crop <= 0 || crop > resize || resize > TV_MAX_SIDE) return p;
    const int lo = (resize - crop) / 2;
    int max_rows = TV_TAPS;
    for (int y0 = 0; y0 < crop; y0 += TV_BAND) {
        const int y1 = std::min(y0 + TV_BAND, crop);
        int first = 0;
        for (int y = y0; y < y1; ++y) {
            int xmin, xmax;
            tv_window(lo + y, n, resize, &xmin, &xmax);
            if (xmax - xmin != TV_TAPS) return p;
            if (y == y0) first = xmin;
            max_rows = std::max(max_rows, xmin + TV_TAPS - first);
        }
    }
    p.crop_p = (crop + 7) / 8 * 8;
    p.max_rows = max_rows;
    p.src_bytes = ((size_t)max_rows * n * chans + 15) / 16 * 16;
    p.lds = (size_t)5 * p.crop_p * sizeof(int) + (size_t)chans * 256 * sizeof(float) + p.src_bytes + (size_t)chans * max_rows * p.crop_p;
    p.ok = p.lds <= (size_t)TV_LDS_BYTES ? 1 : 0;
    return p;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int tv_clip8(int acc) { return clampi(acc >> TV_PREC, 0, 255); }

template <typename T, int COLS> struct tv_store;
template <typename T> struct tv_store<T, 1> {
    static __device__ __forceinline__ void st(T* p, const float (&v)[1]) { io<T>::st(p, v[0]); }
};
template <> struct tv_store<float, 4> {
    static __device__ __forceinline__ void st(float* p, const float (&v)[4]) { io<float>::st4(p, v); }
};
template <> struct tv_store<bf16_t, 8> {
    static __device__ __forceinline__ void st(bf16_t* p, const float (&v)[8]) {
        uint4 t;
        t.x = pack_bf16x2(v[0], v[1]);
        t.y = pack_bf16x2(v[2], v[3]);
        t.z = pack_bf16x2(v[4], v[5]);
        t.w = pack_bf16x2(v[6], v[7]);
        *reinterpret_cast<uint4*>(p) = t;
    }
};

// Workgroup (b, band): output rows [band * TV_BAND, ...) of image b, every channel.  The source rows the band needs are staged as
// they lie; the horizontal pass writes them resampled to `crop` columns as uint8 (Pillow stores that pass as 8 bits), planar, four
// columns per thread as one dword; the vertical pass gives each lane COLS consecutive columns of one output row, lanes running along
// the row and on into the next one, so a wave's stores are 16 bytes per lane to consecutive addresses.  Every table value that becomes
// an address is clamped: a wrong table gives wrong pixels, never a read outside the staged rows.
template <typename T, int COLS>
__global__ __launch_bounds__(TV_THREADS) void teacher_view_kernel(const unsigned char* __restrict__ src, const int64_t* __restrict__ index,
                                                                  const int* __restrict__ table, const float* __restrict__ lut,
                                                                  T* __restrict__ out, int n_src, int C, int n, int crop, int crop_p,
                                                                  int max_rows, int src_bytes) {
    extern __shared__ __align__(16) unsigned char tv_lds[];
    int* tab = reinterpret_cast<int*>(tv_lds);
    float* nl = reinterpret_cast<float*>(tab + 5 * crop_p);
    unsigned char* simg = reinterpret_cast<unsigned char*>(nl + C * 256);
    unsigned char* hb = simg + src_bytes;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int y0 = blockIdx.y * TV_BAND, y1 = min(y0 + TV_BAND, crop), ny = y1 - y0;
    T* o = out + (size_t)b * C * crop * crop;
    const int64_t row = index != nullptr ? index[b] : (int64_t)b;
    if (row < 0 || row >= (int64_t)n_src) {   // workgroup uniform: nothing is read, the band is poisoned
        for (int c = 0; c < C; ++c)
            for (int e = tid; e < ny * crop; e += TV_THREADS) io<T>::st(o + ((size_t)c * crop + y0) * crop + e, __builtin_nanf(""));
        return;
    }
    for (int i = tid; i < 5 * crop_p; i += TV_THREADS) tab[i] = table[i];
    for (int i = tid; i < C * 256; i += TV_THREADS) nl[i] = lut[i];
    const int r0 = clampi(table[y0], 0, n - TV_TAPS);
    const int r1 = clampi(table[y1 - 1], 0, n - TV_TAPS) + TV_TAPS;
    const int nr = min(max(r1 - r0, TV_TAPS), max_rows);
    {
        const unsigned char* g = src + (size_t)row * n * n * C + (size_t)r0 * n * C;
        const int bytes = nr * n * C;
        if (((uintptr_t)g & 3) == 0) {
            const int words = bytes >> 2;
            for (int i = tid; i < words; i += TV_THREADS) reinterpret_cast<unsigned*>(simg)[i] = reinterpret_cast<const unsigned*>(g)[i];
            for (int i = (words << 2) + tid; i < bytes; i += TV_THREADS) simg[i] = g[i];
        } else {
            for (int i = tid; i < bytes; i += TV_THREADS) simg[i] = g[i];
        }
    }
    __syncthreads();

    // horizontal pass over the staged rows
    const int q4 = crop_p >> 2;
    for (int it = tid; it < nr * C * q4; it += TV_THREADS) {
        const int q = it % q4, rc = it / q4;
        const int c = rc % C, r = rc / C;
        const int4 xm = *reinterpret_cast<const int4*>(tab + 4 * q);
        const int4 k0 = *reinterpret_cast<const int4*>(tab + crop_p + 4 * q);
        const int4 k1 = *reinterpret_cast<const int4*>(tab + 2 * crop_p + 4 * q);
        const int4 k2 = *reinterpret_cast<const int4*>(tab + 3 * crop_p + 4 * q);
        const int4 k3 = *reinterpret_cast<const int4*>(tab + 4 * crop_p + 4 * q);
        const int xs[4] = {xm.x, xm.y, xm.z, xm.w};
        const int w0[4] = {k0.x, k0.y, k0.z, k0.w}, w1[4] = {k1.x, k1.y, k1.z, k1.w};
        const int w2[4] = {k2.x, k2.y, k2.z, k2.w}, w3[4] = {k3.x, k3.y, k3.z, k3.w};
        const unsigned char* sr = simg + (size_t)r * n * C + c;
        unsigned packed = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned char* s = sr + clampi(xs[u], 0, n - TV_TAPS) * C;
            const int acc = (1 << (TV_PREC - 1)) + (int)s[0] * w0[u] + (int)s[C] * w1[u] + (int)s[2 * C] * w2[u] + (int)s[3 * C] * w3[u];
            int v = tv_clip8(acc);
            // Kept opaque on purpose.  Left to itself the compiler fuses shift + clamp of two neighbours into one v_ashr_pk_u8_i32 and
            // ORs bytes 2 and 3 into that result's upper half; on the MI355X those two bytes then came out wrong (columns 2 and 3 of
            // every group of four, measured), as if the instruction left bits 31:16 of its destination as they were.
            asm volatile("" : "+v"(v));
            packed |= (unsigned)v << (8 * u);
        }
        *reinterpret_cast<unsigned*>(hb + ((size_t)c * max_rows + r) * crop_p + 4 * q) = packed;
    }
    __syncthreads();

    // vertical pass, normalisation table, store
    const int qn = crop / COLS;   // COLS > 1 only when it divides crop
    for (int it = tid; it < C * ny * qn; it += TV_THREADS) {
        const int q = it % qn, yc = it / qn;
        const int y = y0 + yc % ny, c = yc / ny;
        const int rr = clampi(clampi(tab[y], 0, n - TV_TAPS) - r0, 0, nr - TV_TAPS);
        const int k0 = tab[crop_p + y], k1 = tab[2 * crop_p + y], k2 = tab[3 * crop_p + y], k3 = tab[4 * crop_p + y];
        const unsigned char* h = hb + ((size_t)c * max_rows + rr) * crop_p + COLS * q;
        unsigned char t0[COLS], t1[COLS], t2[COLS], t3[COLS];
        __builtin_memcpy(t0, h, COLS);   // COLS-byte aligned: crop_p is a multiple of 8
        __builtin_memcpy(t1, h + crop_p, COLS);
        __builtin_memcpy(t2, h + 2 * crop_p, COLS);
        __builtin_memcpy(t3, h + 3 * crop_p, COLS);
        const float* nlc = nl + c * 256;
        float v[COLS];
#pragma unroll
        for (int u = 0; u < COLS; ++u) {
            const int acc = (1 << (TV_PREC - 1)) + (int)t0[u] * k0 + (int)t1[u] * k1 + (int)t2[u] * k2 + (int)t3[u] * k3;
            v[u] = nlc[tv_clip8(acc)];
        }
        tv_store<T, COLS>::st(o + ((size_t)c * crop + y) * crop + COLS * q, v);
    }
}

// ================================================================ distillation loss
constexpr int DL_THREADS = 256;
constexpr int DL_WAVES = DL_THREADS / 64;
constexpr int DL_MAX_WG = 64;

// Wave per row, two passes over the row (the second one is served by the cache: a row is 4 * classes bytes).  With q = softmax(z / T),
// p = softmax(t / T) the row's soft term is  sum p (log p - log q).  In general it is taken with every logit shifted by its row's
// maximum:  sum p u - (log s_t - log s_z),  u = ((t - max t) - (z - max z)) / T,  s = the shifted exponential sums -- no term is larger
// than the quantities a log-softmax handles, however far apart the two rows' levels are.  When the two distributions are close (the
// state distillation drives towards) that is a cancellation of two log-sum-exps; with d = (t - z) / T the same term is
// sum p d - log1p(sum q expm1(d)),  exact to fp32 RELATIVE precision for small d: taken when max |d| < 1/2.
// A teacher probability that underflows contributes 0 (the limit), where log(softmax) gives 0 * -inf.
// Rows are joined as in ce_fwd_kernel: per-workgroup partial sums, the last workgroup to arrive adds them in a fixed order and re-arms
// the counter.
// INDEXED (spv_distill_loss_idx_fwd): t is the resident logit cache [n_cache][C] and row r's teacher row is t + index[r] * C -- the one
// difference, so the indexed launch returns the bits of the dense launch on cache[index].  A row whose index lies outside [0, n_cache)
// forms no cache address: the wave runs the row body on the student row in the teacher's place (its CE and the student's two
// log-sum-exps are the true ones) and then poisons what depends on the teacher: the row's soft term and lse3[2][r].
// METER (spv_distill_loss_meter_fwd / _idx_meter_fwd, the training meter of include/spv.h): the walk also finds the student row's first
// maximum and counts the logits ranked in front of the label's (spv_eval_head's rules); the workgroups' hit counts ride behind their
// partials and the joining workgroup logs the step into the meter block.  Every operation that forms lse3 and out3 is the un-metered
// one, in the same order: the instantiations return the same bits.
constexpr int DL_HITS = 2 * DL_MAX_WG + 2;   // first word of the metered workspace's hit partials [DL_MAX_WG][3] (int32)

template <bool INDEXED, bool METER>
__device__ __forceinline__ void distill_fwd_body(const float* __restrict__ z, const float* __restrict__ t,
                                                 const int64_t* __restrict__ index, const int64_t* __restrict__ labels,
                                                 float* __restrict__ lse3, float* __restrict__ out3, float* __restrict__ partial,
                                                 unsigned* __restrict__ counter, int rows, int n_cache, int C, float T, float w_soft,
                                                 float w_ce, long long* meter, int k) {
    __shared__ float ws[2][DL_WAVES];
    __shared__ int hs[METER ? DL_WAVES : 1][3];
    __shared__ bool last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float invT = 1.0f / T;
    float acc_soft = 0.0f, acc_ce = 0.0f;
    int seen = 0, top1 = 0, topk = 0;   // lane 0's
    for (int r = blockIdx.x * DL_WAVES + wave; r < rows; r += gridDim.x * DL_WAVES) {
        const float* zr = z + (size_t)r * C;
        const float* tr = t + (size_t)r * C;
        bool held = true;   // wave uniform
        if constexpr (INDEXED) {
            const int64_t row = index[r];
            held = row >= 0 && row < (int64_t)n_cache;
            tr = held ? t + (size_t)row * C : zr;
        }
        float mz = -INFINITY, mt = -INFINITY, dmax = 0.0f;
        float bm = -INFINITY;   // METER: the lane's first largest student logit and its index (a NaN never wins)
        int am = C;
        int64_t ym = 0;
        float zy = 0.0f;
        if constexpr (METER) {   // the label and its logit first: the two dependent loads are in flight under the first walk of the row
            ym = labels[r];
            zy = zr[(ym >= 0 && ym < C) ? (int)ym : 0];   // clamped, unconditional (one address per wave)
        }
        for (int c = lane; c < C; c += 64) {
            const float a = zr[c], b = tr[c];
            mz = fmaxf(mz, a);
            mt = fmaxf(mt, b);
            dmax = fmaxf(dmax, fabsf((b - a) * invT));
            if constexpr (METER) {
                if (a > bm) { bm = a; am = c; }
            }
        }
        mz = wave_max(mz);
        mt = wave_max(mt);
        dmax = wave_max(dmax);
        const bool nearby = dmax < 0.5f;   // wave uniform
        float s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, pu = 0.0f, qe = 0.0f;
        int first = 0;
        float cnt = 0.0f;
        if constexpr (METER) {
            // the smallest index among the lanes that hold the maximum (indices are below 2^24: exact as floats)
            first = (int)(-wave_max(-(float)((bm == mz && am < C) ? am : C)));
            if (first >= C) first = 0;   // a row without an ordered maximum (every entry NaN or -inf)
        }
        for (int c = lane; c < C; c += 64) {
            const float a = zr[c], b = tr[c];
            if constexpr (METER) cnt += (a > zy || (a == zy && c < ym)) ? 1.0f : 0.0f;
            const float az = (a - mz) * invT, bt = (b - mt) * invT;
            const float ez = expf(az), et = expf(bt);
            const float d = (b - a) * invT;
            s1 += expf(a - mz);
            s2 += ez;
            s3 += et;
            pu += et * (nearby ? d : bt - az);
            qe += ez * expm1f(nearby ? d : 0.0f);
        }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        s3 = wave_sum(s3);
        pu = wave_sum(pu);
        qe = wave_sum(qe);
        const float lz = mz + logf(s1), lzt = mz * invT + logf(s2), ltt = mt * invT + logf(s3);
        const float gap = nearby ? log1pf(qe / s2) : logf(s3) - logf(s2);
        const int64_t y = labels[r];
        if (lane == 0) {
            lse3[r] = lz;
            lse3[rows + r] = lzt;
            lse3[2 * rows + r] = held ? ltt : __builtin_nanf("");
            acc_soft += held ? pu / s3 - gap : __builtin_nanf("");
            acc_ce += (y >= 0 && y < C) ? lz - zr[y] : __builtin_nanf("");   // a label outside [0, C) poisons the loss instead of reading wild
        }
        if constexpr (METER) {
            const int above = (int)wave_sum(cnt);   // at most C < 2^24 ones: exact
            if (lane == 0 && y >= 0 && y < C) {     // a row with a label outside the classes is not counted
                seen += 1;
                top1 += first == (int)y ? 1 : 0;
                topk += above < k ? 1 : 0;
            }
        }
    }
    if (lane == 0) {
        ws[0][wave] = acc_soft;
        ws[1][wave] = acc_ce;
        if constexpr (METER) {
            hs[wave][0] = seen;
            hs[wave][1] = top1;
            hs[wave][2] = topk;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float a = 0.0f, b = 0.0f;
        for (int w = 0; w < DL_WAVES; ++w) {
            a += ws[0][w];
            b += ws[1][w];
        }
        partial[blockIdx.x] = a;
        partial[DL_MAX_WG + blockIdx.x] = b;
        if constexpr (METER) {
            int* hits = reinterpret_cast<int*>(partial + DL_HITS) + 3 * blockIdx.x;
            int a0 = 0, a1 = 0, a2 = 0;
            for (int w = 0; w < DL_WAVES; ++w) {
                a0 += hs[w][0];
                a1 += hs[w][1];
                a2 += hs[w][2];
            }
            hits[0] = a0;
            hits[1] = a1;
            hits[2] = a2;
        }
        __threadfence();
        last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last) {
        __threadfence();
        if (wave == 0) {   // one partial pair per lane (gridDim.x <= 64), joined by the same tree every time
            const bool in = lane < (int)gridDim.x;
            const float a = wave_sum(in ? __builtin_nontemporal_load(partial + lane) : 0.0f);
            const float b = wave_sum(in ? __builtin_nontemporal_load(partial + DL_MAX_WG + lane) : 0.0f);
            float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
            if constexpr (METER) {
                // the hit counts: integers of at most rows <= 2^24 in all, so every float sum below is exact
                const int* hits = reinterpret_cast<const int*>(partial + DL_HITS) + 3 * lane;
                h0 = wave_sum(in ? (float)__builtin_nontemporal_load(hits) : 0.0f);
                h1 = wave_sum(in ? (float)__builtin_nontemporal_load(hits + 1) : 0.0f);
                h2 = wave_sum(in ? (float)__builtin_nontemporal_load(hits + 2) : 0.0f);
            }
            if (lane == 0) {
                const float soft = a * (T * T) / (float)rows, ce = b / (float)rows;
                const float total = w_soft * soft + w_ce * ce;
                out3[0] = total;
                out3[1] = soft;
                out3[2] = ce;
                if constexpr (METER) train_meter_log(meter, total, soft, ce, (int)h0, (int)h1, (int)h2);
                *counter = 0u;
            }
        }
    }
}

template <bool INDEXED>
__global__ __launch_bounds__(DL_THREADS) void distill_fwd_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                                 const int64_t* __restrict__ index, const int64_t* __restrict__ labels,
                                                                 float* __restrict__ lse3, float* __restrict__ out3,
                                                                 float* __restrict__ partial, unsigned* __restrict__ counter, int rows,
                                                                 int n_cache, int C, float T, float w_soft, float w_ce) {
    distill_fwd_body<INDEXED, false>(z, t, index, labels, lse3, out3, partial, counter, rows, n_cache, C, T, w_soft, w_ce, nullptr, 0);
}

template <bool INDEXED>
__global__ __launch_bounds__(DL_THREADS) void distill_meter_fwd_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                                       const int64_t* __restrict__ index, const int64_t* __restrict__ labels,
                                                                       float* __restrict__ lse3, float* __restrict__ out3,
                                                                       float* __restrict__ partial, unsigned* __restrict__ counter, int rows,
                                                                       int n_cache, int C, float T, float w_soft, float w_ce,
                                                                       long long* meter, int k) {
    distill_fwd_body<INDEXED, true>(z, t, index, labels, lse3, out3, partial, counter, rows, n_cache, C, T, w_soft, w_ce, meter, k);
}

// dz = go / rows * (w_soft T (softmax(z / T) - softmax(t / T)) + w_ce (softmax(z) - onehot))
// INDEXED: the teacher's element is t[index[r] * C + c]; a row whose index lies outside [0, n_cache) reads nothing of t and is NaN.
template <bool INDEXED>
__global__ __launch_bounds__(DL_THREADS) void distill_bwd_kernel(const float* __restrict__ z, const float* __restrict__ t,
                                                                 const int64_t* __restrict__ index, const int64_t* __restrict__ labels,
                                                                 const float* __restrict__ lse3, const float* __restrict__ go,
                                                                 float* __restrict__ dz, int rows, int n_cache, int C, float T,
                                                                 float w_soft, float w_ce) {
    const float scale = go[0] / (float)rows, invT = 1.0f / T;
    const float ks = w_soft * T;
    const int64_t total = (int64_t)rows * C;
    for (int64_t e = (int64_t)blockIdx.x * DL_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * DL_THREADS) {
        const int r = (int)(e / C), c = (int)(e - (int64_t)r * C);
        const float a = z[e];
        float b;
        if constexpr (INDEXED) {
            const int64_t row = index[r];
            if (row < 0 || row >= (int64_t)n_cache) {
                dz[e] = __builtin_nanf("");
                continue;
            }
            b = t[(size_t)row * C + c];
        } else {
            b = t[e];
        }
        const float q = expf(a * invT - lse3[rows + r]), p = expf(b * invT - lse3[2 * rows + r]);
        const float s = expf(a - lse3[r]);
        dz[e] = (ks * (q - p) + w_ce * (s - (labels[r] == c ? 1.0f : 0.0f))) * scale;
    }
}

// ================================================================ feature cosine (the hint term, include/spv.h)
constexpr int FC_CHUNK = 8;          // elements a lane takes at a time: 16 bytes of bf16, two 16-byte loads of fp32
constexpr float FC_TINY = 1e-12f;    // F.normalize's eps: below it a norm is "zero" and the row contributes cos = 0, gradient 0

// eight consecutive elements as floats; VEC: 16-byte loads (p 16-byte aligned), else element loads -- the same values either way
template <typename T, bool VEC>
__device__ __forceinline__ void fc_ld8(const T* p, float (&v)[FC_CHUNK]) {
    if constexpr (!VEC) {
#pragma unroll
        for (int u = 0; u < FC_CHUNK; ++u) v[u] = io<T>::ld(p + u);
    } else if constexpr (sizeof(T) == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *(reinterpret_cast<const float4*>(p) + 1);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = __uint_as_float(q.x << 16); v[1] = __uint_as_float(q.x & 0xffff0000u);
        v[2] = __uint_as_float(q.y << 16); v[3] = __uint_as_float(q.y & 0xffff0000u);
        v[4] = __uint_as_float(q.z << 16); v[5] = __uint_as_float(q.z & 0xffff0000u);
        v[6] = __uint_as_float(q.w << 16); v[7] = __uint_as_float(q.w & 0xffff0000u);
    }
}

// Wave per row, one pass: lane l accumulates s.s, t.t, s.t over the chunks l, l + 64, ... and then (l < W % 8) over one element of the
// rest, with explicit fmas -- the order does not depend on VEC, so the aligned and the unaligned launch return the same bits -- and
// the wave reduction joins the lanes.  Rows are joined as in distill_fwd_body: per-workgroup partials, the last workgroup to arrive
// adds them by the same tree every time and re-arms the counter (one exit path).
// INDEXED: t is the resident fp32 feature cache [n_cache][W] and row r's teacher row is t + index[r] * W.  A row whose index lies
// outside [0, n_cache) forms no cache address and reads nothing: its three stats and the loss are NaN.
template <typename TS, typename TT, bool INDEXED, bool VEC>
__global__ __launch_bounds__(DL_THREADS) void feature_cosine_fwd_kernel(const TS* __restrict__ s, const TT* __restrict__ t,
                                                                        const int64_t* __restrict__ index, float* __restrict__ stat3,
                                                                        float* __restrict__ out, float* __restrict__ partial,
                                                                        unsigned* __restrict__ counter, int rows, int n_cache, int W) {
    __shared__ float ws[DL_WAVES];
    __shared__ bool last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = W / FC_CHUNK, rest = W - nch * FC_CHUNK;
    float acc = 0.0f;   // the same in every lane
    for (int r = blockIdx.x * DL_WAVES + wave; r < rows; r += gridDim.x * DL_WAVES) {
        const TS* sr = s + (size_t)r * W;
        const TT* tr = t + (size_t)r * W;
        if constexpr (INDEXED) {
            const int64_t row = index[r];
            if (row < 0 || row >= (int64_t)n_cache) {   // wave uniform
                if (lane == 0) stat3[r] = stat3[rows + r] = stat3[2 * rows + r] = __builtin_nanf("");
                acc += __builtin_nanf("");
                continue;
            }
            tr = t + (size_t)row * W;
        }
        float ss = 0.0f, tt = 0.0f, st = 0.0f;
        for (int j = lane; j < nch; j += 64) {
            float a[FC_CHUNK], b[FC_CHUNK];
            fc_ld8<TS, VEC>(sr + (size_t)j * FC_CHUNK, a);
            fc_ld8<TT, VEC>(tr + (size_t)j * FC_CHUNK, b);
#pragma unroll
            for (int u = 0; u < FC_CHUNK; ++u) {
                ss = fmaf(a[u], a[u], ss);
                tt = fmaf(b[u], b[u], tt);
                st = fmaf(a[u], b[u], st);
            }
        }
        if (lane < rest) {
            const float a = io<TS>::ld(sr + nch * FC_CHUNK + lane), b = io<TT>::ld(tr + nch * FC_CHUNK + lane);
            ss = fmaf(a, a, ss);
            tt = fmaf(b, b, tt);
            st = fmaf(a, b, st);
        }
        ss = wave_sum(ss);
        tt = wave_sum(tt);
        st = wave_sum(st);
        const float ns = sqrtf(ss), nt = sqrtf(tt);
        const float c = (ns < FC_TINY || nt < FC_TINY) ? 0.0f : (st / ns) / nt;   // a NaN norm is not "tiny": it stays NaN
        if (lane == 0) {
            stat3[r] = ns;
            stat3[rows + r] = nt;
            stat3[2 * rows + r] = c;
        }
        acc += c;
    }
    if (lane == 0) ws[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        float a = 0.0f;
        for (int w = 0; w < DL_WAVES; ++w) a += ws[w];
        partial[blockIdx.x] = a;
        __threadfence();
        last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last) {
        __threadfence();
        if (wave == 0) {   // one partial per lane (gridDim.x <= 64)
            const float a = wave_sum(lane < (int)gridDim.x ? __builtin_nontemporal_load(partial + lane) : 0.0f);
            if (lane == 0) {
                out[0] = 1.0f - a / (float)rows;
                *counter = 0u;
            }
        }
    }
}

// ds = -go w / rows * (t / |t| - cos s / |s|) / |s|, V elements per thread (V = 4: W % 4 == 0 and 16-byte aligned bases).  A row with
// a norm below FC_TINY gets zeros; INDEXED: a row whose index lies outside [0, n_cache) reads nothing of t and is NaN.
template <typename TS, typename TT, bool INDEXED, int V>
__global__ __launch_bounds__(DL_THREADS) void feature_cosine_bwd_kernel(const TS* __restrict__ s, const TT* __restrict__ t,
                                                                        const int64_t* __restrict__ index, const float* __restrict__ stat3,
                                                                        const float* __restrict__ go, TS* __restrict__ ds, int rows,
                                                                        int n_cache, int W, float w) {
    const float k = -go[0] * w / (float)rows;
    const int per_row = W / V;
    const int64_t total = (int64_t)rows * per_row;
    for (int64_t e = (int64_t)blockIdx.x * DL_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * DL_THREADS) {
        const int r = (int)(e / per_row), c = (int)(e - (int64_t)r * per_row) * V;
        const size_t at = (size_t)r * W + c;
        float a[V], b[V], o[V];
        size_t tat = at;
        bool held = true;
        if constexpr (INDEXED) {
            const int64_t row = index[r];
            held = row >= 0 && row < (int64_t)n_cache;
            tat = (size_t)row * W + c;   // an offset, not an address: nothing is formed from it unless held
        }
        const float ns = stat3[r], nt = stat3[rows + r], cs = stat3[2 * rows + r];
        if (!held) {
#pragma unroll
            for (int u = 0; u < V; ++u) o[u] = __builtin_nanf("");
        } else if (ns < FC_TINY || nt < FC_TINY) {
#pragma unroll
            for (int u = 0; u < V; ++u) o[u] = 0.0f;
        } else {
            if constexpr (V == 4) {
                io<TS>::ld4(s + at, a);
                io<TT>::ld4(t + tat, b);
            } else {
                a[0] = io<TS>::ld(s + at);
                b[0] = io<TT>::ld(t + tat);
            }
#pragma unroll
            for (int u = 0; u < V; ++u) o[u] = k * ((b[u] / nt - cs * (a[u] / ns)) / ns);
        }
        if constexpr (V == 4) io<TS>::st4(ds + at, o);
        else io<TS>::st(ds + at, o[0]);
    }
}

// ================================================================ resident teacher logits
constexpr int LC_THREADS = 256;

// cache[index[r]][:] = logits[r][:], V floats per lane (V = 4: 16-byte loads and stores, rows of a multiple of 16 bytes at 16-byte
// aligned bases; V = 1: everything else, e.g. 10 classes = 40-byte rows).  A row whose index lies outside [0, n_cache) is skipped:
// nothing is read of it and nothing written.  Plain stores: when an index repeats, one of its rows wins.
template <int V>
__global__ __launch_bounds__(LC_THREADS) void logit_cache_store_kernel(float* __restrict__ cache, const int64_t* __restrict__ index,
                                                                       const float* __restrict__ logits, int rows, int n_cache, int C) {
    const int per_row = C / V;
    const int64_t total = (int64_t)rows * per_row;
    for (int64_t e = (int64_t)blockIdx.x * LC_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * LC_THREADS) {
        const int r = (int)(e / per_row), c = (int)(e - (int64_t)r * per_row) * V;
        const int64_t row = index != nullptr ? index[r] : (int64_t)r;
        if (row < 0 || row >= (int64_t)n_cache) continue;
        const float* s = logits + (size_t)r * C + c;
        float* d = cache + (size_t)row * C + c;
        if constexpr (V == 4) *reinterpret_cast<float4*>(d) = *reinterpret_cast<const float4*>(s);
        else *d = *s;
    }
}

}  // namespace

extern "C" int spv_teacher_view_supported(int chans, int n, int resize, int crop) { return tv_plan(chans, n, resize, crop).ok; }

extern "C" int spv_teacher_view_u8(const unsigned char* src_nhwc, const int64_t* index, const int* table, const float* lut, void* out_nchw,
                                   int batch, int n_src, int chans, int n, int resize, int crop, int dtype, void* stream) {
    SPV_CHECK(batch > 0 && n_src > 0, "spv_teacher_view_u8: bad shape batch=%d n_src=%d", batch, n_src);
    const TvPlan p = tv_plan(chans, n, resize, crop);
    SPV_CHECK(p.ok,
              "spv_teacher_view_u8: %d x %d x %d -> resize %d, crop %d is not supported (1 or 3 channels, 2 <= n <= resize, 0 < crop <= "
              "resize, four taps inside the image for every cropped output, staging within %d bytes of LDS)",
              chans, n, n, resize, crop, TV_LDS_BYTES);
    SPV_CHECK(dtype == SPV_F32 || dtype == SPV_BF16, "spv_teacher_view_u8: bad dtype %d", dtype);
    SPV_CHECK(src_nhwc != nullptr && out_nchw != nullptr, "spv_teacher_view_u8: src / out missing");
    SPV_CHECK(table != nullptr && lut != nullptr, "spv_teacher_view_u8: table / lut missing");
    SPV_CHECK(index != nullptr || batch <= n_src, "spv_teacher_view_u8: index == NULL reads rows 0..batch-1, but batch=%d > n_src=%d", batch,
              n_src);
    SPV_CHECK(((uintptr_t)table & 3) == 0 && ((uintptr_t)lut & 3) == 0 && ((uintptr_t)out_nchw & 3) == 0,
              "spv_teacher_view_u8: table / lut / out must be 4-byte aligned");
    const int bands = cdiv(crop, TV_BAND);
    SPV_CHECK(bands <= 65535, "spv_teacher_view_u8: crop=%d gives too many row bands", crop);
    const bool aligned = ((uintptr_t)out_nchw & 15) == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(batch, bands), block(TV_THREADS);
#define SPV_TV_LAUNCH(TY, COLS)                                                                                                       \
    hipLaunchKernelGGL((teacher_view_kernel<TY, COLS>), grid, block, p.lds, st, src_nhwc, index, table, lut, static_cast<TY*>(out_nchw), \
                       n_src, chans, n, crop, p.crop_p, p.max_rows, (int)p.src_bytes)
    if (dtype == SPV_BF16) {
        if (aligned && crop % 8 == 0) SPV_TV_LAUNCH(bf16_t, 8);
        else SPV_TV_LAUNCH(bf16_t, 1);
    } else {
        if (aligned && crop % 4 == 0) SPV_TV_LAUNCH(float, 4);
        else SPV_TV_LAUNCH(float, 1);
    }
#undef SPV_TV_LAUNCH
    SPV_LAUNCH_CHECK("spv_teacher_view_u8");
    SPV_COUNT_PATH(SPV_PATH_TEACHER_VIEW);
    return 0;
}

extern "C" int64_t spv_distill_loss_workspace_floats() { return 2 * DL_MAX_WG + 1; }   // two partial sums per workgroup + the arrival counter

static int distill_check(const char* name, const void* a, const void* b, const void* c, const void* d, const void* e, const void* f, int rows,
                         int classes, float T, float w_soft, float w_ce) {
    SPV_CHECK(rows > 0 && classes > 0, "%s: empty (rows=%d classes=%d)", name, rows, classes);
    SPV_CHECK(T > 0.0f && std::isfinite(T), "%s: temperature T=%g must be positive and finite", name, (double)T);
    SPV_CHECK(std::isfinite(w_soft) && std::isfinite(w_ce), "%s: a loss weight is not finite", name);
    SPV_CHECK(a != nullptr && b != nullptr && c != nullptr, "%s: student / teacher / labels missing", name);
    SPV_CHECK(d != nullptr && e != nullptr && f != nullptr, "%s: an output or workspace pointer is missing", name);
    return 0;
}

extern "C" int spv_distill_loss_fwd(const float* student, const float* teacher, const int64_t* labels, float* lse3, float* out3,
                                    float* workspace, int rows, int classes, float T, float w_soft, float w_ce, void* stream) {
    if (int rc = distill_check("spv_distill_loss_fwd", student, teacher, labels, lse3, out3, workspace, rows, classes, T, w_soft, w_ce)) return rc;
    const int wgs = std::min(cdiv(rows, DL_WAVES), DL_MAX_WG);
    hipLaunchKernelGGL(distill_fwd_kernel<false>, dim3(wgs), dim3(DL_THREADS), 0, static_cast<hipStream_t>(stream), student, teacher,
                       (const int64_t*)nullptr, labels, lse3, out3, workspace, reinterpret_cast<unsigned*>(workspace + 2 * DL_MAX_WG), rows,
                       0, classes, T, w_soft, w_ce);
    SPV_LAUNCH_CHECK("spv_distill_loss_fwd");
    return 0;
}

extern "C" int spv_distill_loss_bwd(const float* student, const float* teacher, const int64_t* labels, const float* lse3,
                                    const float* grad_out, float* dlogits, int rows, int classes, float T, float w_soft, float w_ce,
                                    void* stream) {
    if (int rc = distill_check("spv_distill_loss_bwd", student, teacher, labels, lse3, grad_out, dlogits, rows, classes, T, w_soft, w_ce)) return rc;
    const int64_t total = (int64_t)rows * classes;
    hipLaunchKernelGGL(distill_bwd_kernel<false>, dim3((unsigned)std::min<int64_t>((total + DL_THREADS - 1) / DL_THREADS, 1024)),
                       dim3(DL_THREADS), 0, static_cast<hipStream_t>(stream), student, teacher, (const int64_t*)nullptr, labels, lse3, grad_out,
                       dlogits, rows, 0, classes, T, w_soft, w_ce);
    SPV_LAUNCH_CHECK("spv_distill_loss_bwd");
    return 0;
}

// ---- the same loss with the teacher's rows read from the resident cache through the batch's index
static int distill_idx_check(const char* name, const void* index, int n_cache) {
    SPV_CHECK(index != nullptr, "%s: index missing", name);
    SPV_CHECK(n_cache > 0, "%s: empty cache (n_cache=%d)", name, n_cache);
    return 0;
}

extern "C" int spv_distill_loss_idx_fwd(const float* student, const float* cache, const int64_t* index, const int64_t* labels, float* lse3,
                                        float* out3, float* workspace, int rows, int n_cache, int classes, float T, float w_soft, float w_ce,
                                        void* stream) {
    if (int rc = distill_check("spv_distill_loss_idx_fwd", student, cache, labels, lse3, out3, workspace, rows, classes, T, w_soft, w_ce)) return rc;
    if (int rc = distill_idx_check("spv_distill_loss_idx_fwd", index, n_cache)) return rc;
    const int wgs = std::min(cdiv(rows, DL_WAVES), DL_MAX_WG);
    hipLaunchKernelGGL(distill_fwd_kernel<true>, dim3(wgs), dim3(DL_THREADS), 0, static_cast<hipStream_t>(stream), student, cache, index,
                       labels, lse3, out3, workspace, reinterpret_cast<unsigned*>(workspace + 2 * DL_MAX_WG), rows, n_cache, classes, T,
                       w_soft, w_ce);
    SPV_LAUNCH_CHECK("spv_distill_loss_idx_fwd");
    SPV_COUNT_PATH(SPV_PATH_DISTILL_CACHED);
    return 0;
}

extern "C" int spv_distill_loss_idx_bwd(const float* student, const float* cache, const int64_t* index, const int64_t* labels,
                                        const float* lse3, const float* grad_out, float* dlogits, int rows, int n_cache, int classes, float T,
                                        float w_soft, float w_ce, void* stream) {
    if (int rc = distill_check("spv_distill_loss_idx_bwd", student, cache, labels, lse3, grad_out, dlogits, rows, classes, T, w_soft, w_ce)) return rc;
    if (int rc = distill_idx_check("spv_distill_loss_idx_bwd", index, n_cache)) return rc;
    const int64_t total = (int64_t)rows * classes;
    hipLaunchKernelGGL(distill_bwd_kernel<true>, dim3((unsigned)std::min<int64_t>((total + DL_THREADS - 1) / DL_THREADS, 1024)),
                       dim3(DL_THREADS), 0, static_cast<hipStream_t>(stream), student, cache, index, labels, lse3, grad_out, dlogits, rows,
                       n_cache, classes, T, w_soft, w_ce);
    SPV_LAUNCH_CHECK("spv_distill_loss_idx_bwd");
    return 0;
}

// ---- the feature cosine term, dense and through the resident feature cache
extern "C" int64_t spv_feature_cosine_workspace_floats() { return DL_MAX_WG + 1; }   // a partial sum per workgroup + the arrival counter

static inline size_t fc_es(int dtype) { return dtype == SPV_BF16 ? 2 : 4; }

static int feature_check(const char* name, const void* a, const void* b, const void* c, const void* d, const void* e, int rows, int width,
                         int s_dtype, int t_dtype, float w) {
    SPV_CHECK(rows > 0 && width > 0, "%s: empty (rows=%d width=%d)", name, rows, width);
    SPV_CHECK(rows <= (1 << 24), "%s: rows=%d above 2^24 (the mean's divisor is an exact fp32 integer)", name, rows);
    SPV_CHECK((s_dtype == SPV_F32 || s_dtype == SPV_BF16) && (t_dtype == SPV_F32 || t_dtype == SPV_BF16),
              "%s: bad dtype (student %d, teacher %d): SPV_F32 or SPV_BF16", name, s_dtype, t_dtype);
    SPV_CHECK(std::isfinite(w), "%s: the weight is not finite", name);
    SPV_CHECK(a != nullptr && b != nullptr, "%s: student / teacher missing", name);
    SPV_CHECK(c != nullptr && d != nullptr && e != nullptr, "%s: an output, stat3, grad_out or workspace pointer is missing", name);
    SPV_CHECK((uintptr_t)a % fc_es(s_dtype) == 0 && (uintptr_t)b % fc_es(t_dtype) == 0, "%s: student / teacher not aligned to their elements",
              name);
    return 0;
}

// both operands readable as 16-byte chunks: both bases and both row pitches multiples of 16 bytes
static inline bool fc_vec(const void* s, const void* t, int width, int s_dtype, int t_dtype) {
    return (((uintptr_t)s | (uintptr_t)t) & 15) == 0 && (width * fc_es(s_dtype)) % 16 == 0 && (width * fc_es(t_dtype)) % 16 == 0;
}

template <bool INDEXED>
static void feature_fwd_launch(const void* s, const void* t, const int64_t* index, float* stat3, float* out, float* workspace, int rows,
                               int n_cache, int width, int s_dtype, int t_dtype, hipStream_t st) {
    const dim3 grid(std::min(cdiv(rows, DL_WAVES), DL_MAX_WG)), block(DL_THREADS);
    unsigned* counter = reinterpret_cast<unsigned*>(workspace + DL_MAX_WG);
    const bool vec = fc_vec(s, t, width, s_dtype, t_dtype);
#define SPV_FC_FWD(TS, TT)                                                                                                               \
    do {                                                                                                                                 \
        if (vec)                                                                                                                         \
            hipLaunchKernelGGL((feature_cosine_fwd_kernel<TS, TT, INDEXED, true>), grid, block, 0, st, static_cast<const TS*>(s),         \
                               static_cast<const TT*>(t), index, stat3, out, workspace, counter, rows, n_cache, width);                  \
        else                                                                                                                             \
            hipLaunchKernelGGL((feature_cosine_fwd_kernel<TS, TT, INDEXED, false>), grid, block, 0, st, static_cast<const TS*>(s),        \
                               static_cast<const TT*>(t), index, stat3, out, workspace, counter, rows, n_cache, width);                  \
    } while (0)
    if constexpr (INDEXED) {   // the cache is fp32
        if (s_dtype == SPV_BF16) SPV_FC_FWD(bf16_t, float);
        else SPV_FC_FWD(float, float);
    } else {
        if (s_dtype == SPV_BF16 && t_dtype == SPV_BF16) SPV_FC_FWD(bf16_t, bf16_t);
        else if (s_dtype == SPV_BF16) SPV_FC_FWD(bf16_t, float);
        else if (t_dtype == SPV_BF16) SPV_FC_FWD(float, bf16_t);
        else SPV_FC_FWD(float, float);
    }
#undef SPV_FC_FWD
}

template <bool INDEXED>
static void feature_bwd_launch(const void* s, const void* t, const int64_t* index, const float* stat3, const float* go, void* ds, int rows,
                               int n_cache, int width, int s_dtype, int t_dtype, float w, hipStream_t st) {
    const bool vec = width % 4 == 0 && (((uintptr_t)s | (uintptr_t)t | (uintptr_t)ds) & 15) == 0;
    const int64_t total = (int64_t)rows * (vec ? width / 4 : width);
    const dim3 grid((unsigned)std::min<int64_t>((total + DL_THREADS - 1) / DL_THREADS, 1024)), block(DL_THREADS);
#define SPV_FC_BWD(TS, TT)                                                                                                               \
    do {                                                                                                                                 \
        if (vec)                                                                                                                         \
            hipLaunchKernelGGL((feature_cosine_bwd_kernel<TS, TT, INDEXED, 4>), grid, block, 0, st, static_cast<const TS*>(s),            \
                               static_cast<const TT*>(t), index, stat3, go, static_cast<TS*>(ds), rows, n_cache, width, w);              \
        else                                                                                                                             \
            hipLaunchKernelGGL((feature_cosine_bwd_kernel<TS, TT, INDEXED, 1>), grid, block, 0, st, static_cast<const TS*>(s),            \
                               static_cast<const TT*>(t), index, stat3, go, static_cast<TS*>(ds), rows, n_cache, width, w);              \
    } while (0)
    if constexpr (INDEXED) {
        if (s_dtype == SPV_BF16) SPV_FC_BWD(bf16_t, float);
        else SPV_FC_BWD(float, float);
    } else {
        if (s_dtype == SPV_BF16 && t_dtype == SPV_BF16) SPV_FC_BWD(bf16_t, bf16_t);
        else if (s_dtype == SPV_BF16) SPV_FC_BWD(bf16_t, float);
        else if (t_dtype == SPV_BF16) SPV_FC_BWD(float, bf16_t);
        else SPV_FC_BWD(float, float);
    }
#undef SPV_FC_BWD
}

extern "C" int spv_feature_cosine_fwd(const void* student, const void* teacher, float* stat3, float* out, float* workspace, int rows,
                                      int width, int s_dtype, int t_dtype, void* stream) {
    if (int rc = feature_check("spv_feature_cosine_fwd", student, teacher, stat3, out, workspace, rows, width, s_dtype, t_dtype, 0.0f)) return rc;
    feature_fwd_launch<false>(student, teacher, nullptr, stat3, out, workspace, rows, 0, width, s_dtype, t_dtype, static_cast<hipStream_t>(stream));
    SPV_LAUNCH_CHECK("spv_feature_cosine_fwd");
    return 0;
}

extern "C" int spv_feature_cosine_bwd(const void* student, const void* teacher, const float* stat3, const float* grad_out, void* dstudent,
                                      int rows, int width, int s_dtype, int t_dtype, float w, void* stream) {
    if (int rc = feature_check("spv_feature_cosine_bwd", student, teacher, stat3, grad_out, dstudent, rows, width, s_dtype, t_dtype, w)) return rc;
    SPV_CHECK((uintptr_t)dstudent % fc_es(s_dtype) == 0, "spv_feature_cosine_bwd: dstudent not aligned to its elements");
    feature_bwd_launch<false>(student, teacher, nullptr, stat3, grad_out, dstudent, rows, 0, width, s_dtype, t_dtype, w,
                              static_cast<hipStream_t>(stream));
    SPV_LAUNCH_CHECK("spv_feature_cosine_bwd");
    return 0;
}

extern "C" int spv_feature_cosine_idx_fwd(const void* student, const float* cache, const int64_t* index, float* stat3, float* out,
                                          float* workspace, int rows, int n_cache, int width, int s_dtype, void* stream) {
    if (int rc = feature_check("spv_feature_cosine_idx_fwd", student, cache, stat3, out, workspace, rows, width, s_dtype, SPV_F32, 0.0f)) return rc;
    if (int rc = distill_idx_check("spv_feature_cosine_idx_fwd", index, n_cache)) return rc;
    feature_fwd_launch<true>(student, cache, index, stat3, out, workspace, rows, n_cache, width, s_dtype, SPV_F32, static_cast<hipStream_t>(stream));
    SPV_LAUNCH_CHECK("spv_feature_cosine_idx_fwd");
    return 0;
}

extern "C" int spv_feature_cosine_idx_bwd(const void* student, const float* cache, const int64_t* index, const float* stat3,
                                          const float* grad_out, void* dstudent, int rows, int n_cache, int width, int s_dtype, float w,
                                          void* stream) {
    if (int rc = feature_check("spv_feature_cosine_idx_bwd", student, cache, stat3, grad_out, dstudent, rows, width, s_dtype, SPV_F32, w)) return rc;
    if (int rc = distill_idx_check("spv_feature_cosine_idx_bwd", index, n_cache)) return rc;
    SPV_CHECK((uintptr_t)dstudent % fc_es(s_dtype) == 0, "spv_feature_cosine_idx_bwd: dstudent not aligned to its elements");
    feature_bwd_launch<true>(student, cache, index, stat3, grad_out, dstudent, rows, n_cache, width, s_dtype, SPV_F32, w,
                             static_cast<hipStream_t>(stream));
    SPV_LAUNCH_CHECK("spv_feature_cosine_idx_bwd");
    return 0;
}

// ---- the training meter (include/spv.h): the same two forwards, counting hits and logging the step
extern "C" int64_t spv_distill_loss_meter_workspace_floats() { return DL_HITS + 3 * DL_MAX_WG; }   // + one word of padding, the hit partials

extern "C" int spv_distill_loss_meter_fwd(const float* student, const float* teacher, const int64_t* labels, float* lse3, float* out3,
                                          float* workspace, int rows, int classes, float T, float w_soft, float w_ce, void* meter, int k,
                                          void* stream) {
    if (int rc = distill_check("spv_distill_loss_meter_fwd", student, teacher, labels, lse3, out3, workspace, rows, classes, T, w_soft, w_ce)) return rc;
    if (int rc = spv_train_meter_check("spv_distill_loss_meter_fwd", meter, k, rows, classes)) return rc;
    const int wgs = std::min(cdiv(rows, DL_WAVES), DL_MAX_WG);   // spv_distill_loss_fwd's grid: the same partial order
    hipLaunchKernelGGL(distill_meter_fwd_kernel<false>, dim3(wgs), dim3(DL_THREADS), 0, static_cast<hipStream_t>(stream), student, teacher,
                       (const int64_t*)nullptr, labels, lse3, out3, workspace, reinterpret_cast<unsigned*>(workspace + 2 * DL_MAX_WG), rows,
                       0, classes, T, w_soft, w_ce, static_cast<long long*>(meter), k);
    SPV_LAUNCH_CHECK("spv_distill_loss_meter_fwd");
    return 0;
}

extern "C" int spv_distill_loss_idx_meter_fwd(const float* student, const float* cache, const int64_t* index, const int64_t* labels,
                                              float* lse3, float* out3, float* workspace, int rows, int n_cache, int classes, float T,
                                              float w_soft, float w_ce, void* meter, int k, void* stream) {
    if (int rc = distill_check("spv_distill_loss_idx_meter_fwd", student, cache, labels, lse3, out3, workspace, rows, classes, T, w_soft, w_ce)) return rc;
    if (int rc = distill_idx_check("spv_distill_loss_idx_meter_fwd", index, n_cache)) return rc;
    if (int rc = spv_train_meter_check("spv_distill_loss_idx_meter_fwd", meter, k, rows, classes)) return rc;
    const int wgs = std::min(cdiv(rows, DL_WAVES), DL_MAX_WG);
    hipLaunchKernelGGL(distill_meter_fwd_kernel<true>, dim3(wgs), dim3(DL_THREADS), 0, static_cast<hipStream_t>(stream), student, cache, index,
                       labels, lse3, out3, workspace, reinterpret_cast<unsigned*>(workspace + 2 * DL_MAX_WG), rows, n_cache, classes, T,
                       w_soft, w_ce, static_cast<long long*>(meter), k);
    SPV_LAUNCH_CHECK("spv_distill_loss_idx_meter_fwd");
    SPV_COUNT_PATH(SPV_PATH_DISTILL_CACHED);
    return 0;
}

extern "C" int spv_logit_cache_store(float* cache, const int64_t* index, const float* logits, int rows, int n_cache, int classes,
                                     void* stream) {
    SPV_CHECK(rows > 0 && n_cache > 0 && classes > 0, "spv_logit_cache_store: empty (rows=%d n_cache=%d classes=%d)", rows, n_cache, classes);
    SPV_CHECK(cache != nullptr && logits != nullptr, "spv_logit_cache_store: cache / logits missing");
    SPV_CHECK(index != nullptr || rows <= n_cache, "spv_logit_cache_store: index == NULL writes rows 0..rows-1, but rows=%d > n_cache=%d", rows,
              n_cache);
    SPV_CHECK(((uintptr_t)cache & 3) == 0 && ((uintptr_t)logits & 3) == 0, "spv_logit_cache_store: cache / logits must be 4-byte aligned");
    const bool vec = classes % 4 == 0 && (((uintptr_t)cache | (uintptr_t)logits) & 15) == 0;
    const int64_t total = (int64_t)rows * (vec ? classes / 4 : classes);
    const dim3 grid((unsigned)std::min<int64_t>((total + LC_THREADS - 1) / LC_THREADS, 1024)), block(LC_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(logit_cache_store_kernel<4>, grid, block, 0, st, cache, index, logits, rows, n_cache, classes);
    else hipLaunchKernelGGL(logit_cache_store_kernel<1>, grid, block, 0, st, cache, index, logits, rows, n_cache, classes);
    SPV_LAUNCH_CHECK("spv_logit_cache_store");
    return 0;
}
