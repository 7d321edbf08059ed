// spv_dataset_ingest (include/spv.h): a dataset file's uint8 pixel payload, uploaded as it is, written in the other
// layout (planar [n][c][h][w] <-> interleaved [n][h][w][c]) with the set's statistics taken in the same walk.  A workgroup takes a unit:
// a group of whole small images, or one tile of pixels of a large one.  A unit is ONE contiguous run of bytes on its interleaved side and
// one (whole images) or c (a tile) runs on its planar side; the source runs are staged in LDS at offsets congruent to their global
// addresses mod 16, so 16-byte global accesses meet 16-byte LDS accesses whatever the pointers' alignment, with byte accesses for a
// run's unaligned head and tail.  The destination walk reads single bytes from LDS, packs 16 and stores them at once, and feeds the
// sums.  A workgroup keeps its sums (64-bit, in registers) and its label histogram (LDS, up to ING_HIST classes) across the units it
// walks and adds them to `stats` once at its end: adds to one address serialise, so their count per address is the grid's size and not
// the units' or the labels'.  Everything is integer: the statistics do not depend on the order of the adds.  Plain C++, vector atomics
// from atomicAdd.
#include "spv_common.h"

namespace {

constexpr int ING_THREADS = 256;
constexpr int ING_WAVES = ING_THREADS / 64;
constexpr int ING_TILE = 8192;              // pixels of a unit at the most
constexpr int ING_RUN = ING_TILE + 16;      // LDS bytes of a planar tile's run: its bytes and the (address & 15) in front of them
constexpr int ING_LDS = 3 * ING_RUN;
constexpr int ING_MAX_GRID = 1024;          // workgroups of a launch (four per CU); further units are walked by the same ones
constexpr int ING_HIST = 1024;              // classes up to which a workgroup keeps its label histogram in LDS
// a unit's sum of x^2 per channel stays below 2^32 (66 051 pixels could meet there): the sums inside a unit are 32-bit, everything
// that crosses units -- the adds into `stats` -- is 64-bit
static_assert((unsigned long long)ING_TILE * 255ull * 255ull < (1ull << 32), "a unit's sum of squares must fit 32 bits");

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // lane 0 holds the wave's sum
}

// `len` bytes from global `src` to LDS at `at` (at == src mod 16): head bytes, 16-byte body, tail bytes
__device__ __forceinline__ void stage_run(const unsigned char* __restrict__ src, unsigned char* lds, int at, int len, int tid) {
    int head = (int)((16u - (unsigned)((uintptr_t)src & 15)) & 15);
    if (head > len) head = len;
    const int nvec = (len - head) >> 4;
    const uint4* s = reinterpret_cast<const uint4*>(src + head);
    uint4* d = reinterpret_cast<uint4*>(lds + at + head);
    for (int k = tid; k < nvec; k += ING_THREADS) d[k] = s[k];
    const int tail_at = head + (nvec << 4);
    const int loose = head + (len - tail_at);   // < 32
    if (tid < loose) {
        const int j = tid < head ? tid : tail_at + (tid - head);
        lds[at + j] = src[j];
    }
}

template <int C> struct Sums {
    unsigned s[C], q[C];
    __device__ __forceinline__ void add(int ch, unsigned x) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const unsigned y = ch == k ? x : 0u;
            s[k] += y;
            q[k] += y * y;
        }
    }
};

// the LDS position of destination byte v of the unit.  TO_PLANAR (source interleaved, one staged run at `base[0]`): v = (g * C + ch) * pt
// + p.  Otherwise (source planar, channel ch's bytes of image g at base[ch] + g * C * pt): v = (g * pt + p) * C + ch.
template <int C, bool TO_PLANAR> struct Walk {
    int g, ch, p, pt;
    __device__ __forceinline__ Walk(int v, int pt_) : pt(pt_) {
        if (TO_PLANAR) {
            const int plane = v / pt;
            p = v - plane * pt;
            g = plane / C;
            ch = plane - g * C;
        } else {
            const int pix = v / C;
            ch = v - pix * C;
            g = pix / pt;
            p = pix - g * pt;
        }
    }
    __device__ __forceinline__ int pos(const int* base) const {
        return TO_PLANAR ? base[0] + (g * pt + p) * C + ch : base[ch] + g * C * pt + p;
    }
    __device__ __forceinline__ void next() {
        if (TO_PLANAR) {
            if (++p == pt) {
                p = 0;
                if (++ch == C) { ch = 0; ++g; }
            }
        } else {
            if (++ch == C) {
                ch = 0;
                if (++p == pt) { p = 0; ++g; }
            }
        }
    }
};

// destination bytes [v0, v0 + len) of the unit: read from LDS, counted, and (dst: the global address of byte v0, or null) stored
template <int C, bool TO_PLANAR>
__device__ __forceinline__ void emit_run(unsigned char* __restrict__ dst, const unsigned char* lds, const int* base, int v0, int len, int pt,
                                         int tid, Sums<C>& sums) {
    int head = dst ? (int)((16u - (unsigned)((uintptr_t)dst & 15)) & 15) : 0;
    if (head > len) head = len;
    const int nvec = (len - head) >> 4;
    for (int k = tid; k < nvec; k += ING_THREADS) {
        const int j = head + (k << 4);
        Walk<C, TO_PLANAR> w(v0 + j, pt);
        unsigned word[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned acc = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned x = lds[w.pos(base)];
                sums.add(w.ch, x);
                acc |= x << (8 * b);
                w.next();
            }
            word[i] = acc;
        }
        if (dst) *reinterpret_cast<uint4*>(dst + j) = make_uint4(word[0], word[1], word[2], word[3]);
    }
    const int tail_at = head + (nvec << 4);
    const int loose = head + (len - tail_at);   // < 32
    if (tid < loose) {
        const int j = tid < head ? tid : tail_at + (tid - head);
        Walk<C, TO_PLANAR> w(v0 + j, pt);
        const unsigned x = lds[w.pos(base)];
        sums.add(w.ch, x);
        if (dst) dst[j] = (unsigned char)x;
    }
}

// group: images of a unit (hw <= ING_TILE: whole images, one unit per group); tiles: units of an image (hw > ING_TILE: group == 1)
template <int C, bool TO_PLANAR>
__global__ __launch_bounds__(ING_THREADS) void dataset_ingest_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                     const unsigned char* __restrict__ labels, int label_i64,
                                                                     unsigned long long* __restrict__ stats, long long n, int hw, int group,
                                                                     int tiles, long long units, int classes) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[ING_LDS];
    __shared__ unsigned red[ING_WAVES][2 * C];
    __shared__ unsigned hist[ING_HIST];
    __shared__ unsigned stray;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long image_bytes = (long long)C * hw;
    const bool lds_hist = labels && classes <= ING_HIST;
    unsigned long long total = 0;   // thread k < 2 C: statistic k of this workgroup's units; thread 2 C: their pixels
    if (lds_hist) {
        for (int b = tid; b < classes; b += ING_THREADS) hist[b] = 0;
        if (tid == 0) stray = 0;
    }   // (the first unit's barrier behind the staging orders these stores in front of every add)

    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        long long n0;
        int images, p0, pt;
        if (tiles == 1) {
            n0 = u * group;
            images = (int)(n - n0 < group ? n - n0 : group);
            p0 = 0;
            pt = hw;
        } else {
            n0 = u / tiles;
            images = 1;
            p0 = (int)(u - n0 * tiles) * ING_TILE;
            pt = hw - p0 < ING_TILE ? hw - p0 : ING_TILE;
        }
        const bool whole = tiles == 1;   // the unit is one contiguous run on both sides
        const unsigned char* s0 = src + n0 * image_bytes;
        int base[3] = {0, 0, 0};
        if (TO_PLANAR || whole) {   // one staged run: interleaved bytes, or whole planar images
            const unsigned char* s = s0 + (TO_PLANAR ? (long long)p0 * C : 0);
            base[0] = (int)((uintptr_t)s & 15);
            stage_run(s, lds, base[0], images * C * pt, tid);
            if (!TO_PLANAR) {
#pragma unroll
                for (int k = 1; k < C; ++k) base[k] = base[0] + k * pt;
            }
        } else {   // a tile of a large planar image: a run per channel
#pragma unroll
            for (int k = 0; k < C; ++k) {
                const unsigned char* s = s0 + (long long)k * hw + p0;
                base[k] = k * ING_RUN + (int)((uintptr_t)s & 15);
                stage_run(s, lds, base[k], pt, tid);
            }
        }
        __syncthreads();

        Sums<C> sums;
#pragma unroll
        for (int k = 0; k < C; ++k) sums.s[k] = sums.q[k] = 0;
        unsigned char* d0 = dst ? dst + n0 * image_bytes : nullptr;
        if (!TO_PLANAR || whole) {
            unsigned char* d = d0 ? d0 + (TO_PLANAR ? 0 : (long long)p0 * C) : nullptr;
            emit_run<C, TO_PLANAR>(d, lds, base, 0, images * C * pt, pt, tid, sums);
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k)
                emit_run<C, TO_PLANAR>(d0 ? d0 + (long long)k * hw + p0 : nullptr, lds, base, k * pt, pt, pt, tid, sums);
        }

        // the unit's sums: a wave reduction each, the waves' results through LDS into the workgroup's 64-bit totals
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const unsigned a = wave_sum(sums.s[k]), b = wave_sum(sums.q[k]);
            if (lane == 0) {
                red[wave][k] = a;
                red[wave][C + k] = b;
            }
        }
        __syncthreads();   // (also: every read of the staged bytes is done before the next unit overwrites them)
        if (tid < 2 * C) {
#pragma unroll
            for (int wv = 0; wv < ING_WAVES; ++wv) total += red[wv][tid];
        }
        if (tid == 2 * C) total += (unsigned long long)images * (unsigned long long)pt;

        if (labels && p0 == 0) {   // the labels of the unit's images (read bytewise: any alignment)
            for (int i = tid; i < images; i += ING_THREADS) {
                long long v;
                if (label_i64) {
                    const unsigned char* l = labels + 8 * (n0 + i);
                    unsigned long long bits = 0;
#pragma unroll
                    for (int b = 0; b < 8; ++b) bits |= (unsigned long long)l[b] << (8 * b);
                    v = (long long)bits;
                } else {
                    v = labels[n0 + i];
                }
                const bool inside = v >= 0 && v < classes;
                if (lds_hist) {
                    atomicAdd(inside ? &hist[v] : &stray, 1u);
                } else {
                    atomicAdd(&stats[inside ? 2 * C + 2 + v : 2 * C + 1], 1ull);
                }
            }
        }
    }
    // the workgroup's one add per statistic, and per class it met
    if (tid <= 2 * C) atomicAdd(&stats[tid], total);
    if (lds_hist) {
        __syncthreads();
        for (int b = tid; b < classes; b += ING_THREADS)
            if (hist[b]) atomicAdd(&stats[2 * C + 2 + b], (unsigned long long)hist[b]);
        if (tid == 0 && stray) atomicAdd(&stats[2 * C + 1], (unsigned long long)stray);
    }
}

template <int C, bool TO_PLANAR>
void launch_ingest(const unsigned char* src, unsigned char* dst, const void* labels, int label_dtype, unsigned long long* stats, long long n,
                   int hw, int classes, hipStream_t stream) {
    const int group = hw <= ING_TILE ? ING_TILE / hw : 1;
    const int tiles = hw <= ING_TILE ? 1 : (hw + ING_TILE - 1) / ING_TILE;
    const long long units = tiles == 1 ? (n + group - 1) / group : n * tiles;
    const int grid = (int)(units < ING_MAX_GRID ? units : ING_MAX_GRID);
    hipLaunchKernelGGL((dataset_ingest_kernel<C, TO_PLANAR>), dim3(grid), dim3(ING_THREADS), 0, stream, src, dst,
                       static_cast<const unsigned char*>(labels), label_dtype == SPV_LOADER_LABEL_I64, stats, n, hw, group, tiles, units,
                       classes);
}

}  // namespace

extern "C" int64_t spv_dataset_stats_words(int c, int classes) {
    if (c < 1 || classes < 0) return 0;
    return 2 * (int64_t)c + 2 + classes;
}

extern "C" int spv_dataset_ingest(const uint8_t* src, uint8_t* dst, const void* labels, int label_dtype, uint64_t* stats, int64_t n, int c,
                                  int h, int w, int src_layout, int classes, void* stream) {
    SPV_CHECK(c == 1 || c == 3, "spv_dataset_ingest: c = %d (1 or 3 channels)", c);
    SPV_CHECK(h >= 1 && h <= 512 && w >= 1 && w <= 512, "spv_dataset_ingest: h = %d, w = %d (sides 1 .. 512)", h, w);
    SPV_CHECK(n >= 0 && n < (1ll << 31), "spv_dataset_ingest: n = %lld (0 <= n < 2^31)", (long long)n);
    SPV_CHECK(src_layout == SPV_DATASET_PLANAR || src_layout == SPV_DATASET_INTERLEAVED, "spv_dataset_ingest: src_layout = %d", src_layout);
    SPV_CHECK(classes >= 0 && classes <= (1 << 24), "spv_dataset_ingest: classes = %d (0 .. 2^24)", classes);
    SPV_CHECK(label_dtype == SPV_LOADER_LABEL_U8 || label_dtype == SPV_LOADER_LABEL_I64, "spv_dataset_ingest: label_dtype = %d", label_dtype);
    SPV_CHECK(stats && ((uintptr_t)stats & 7) == 0, "spv_dataset_ingest: stats is null or not 8-byte aligned");
    if (n == 0) return 0;
    SPV_CHECK(src, "spv_dataset_ingest: null src");
    const long long bytes = (long long)n * c * h * w;
    if (dst) {
        const uintptr_t a = (uintptr_t)src, b = (uintptr_t)dst;
        SPV_CHECK(a + (uintptr_t)bytes <= b || b + (uintptr_t)bytes <= a, "spv_dataset_ingest: src and dst overlap (not an in-place call)");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(stats);
    const bool to_planar = src_layout == SPV_DATASET_INTERLEAVED;
    if (c == 1) {   // one channel: the two layouts are the same bytes; the planar walk copies them
        launch_ingest<1, true>(src, dst, labels, label_dtype, words, n, h * w, classes, st);
    } else if (to_planar) {
        launch_ingest<3, true>(src, dst, labels, label_dtype, words, n, h * w, classes, st);
    } else {
        launch_ingest<3, false>(src, dst, labels, label_dtype, words, n, h * w, classes, st);
    }
    SPV_LAUNCH_CHECK("spv_dataset_ingest");
    return 0;
}
