// The resident loader's fetch (include/spv.h "the resident loader"): ONE launch reads the step from a device
// cursor, writes that step's batch -- index, labels, image -- to fixed addresses and advances the cursor.  Nothing of it is a by-value
// function of the step, so a captured launch fetches a new batch at every replay.
#include "spv_common.h"
#include "spv_loader_core.h"

namespace {

static_assert(LDR_ROUNDS == SPV_LOADER_ROUNDS, "spv_loader_core.h and include/spv.h state the same network");
constexpr int LT = 256;                   // threads of a workgroup
constexpr int LDR_SPAN_PX = 4 * LT;       // float mode: pixels of one workgroup's span (four per thread and channel)
constexpr int LDR_SPAN_BYTES = 16 * LT;   // uint8 mode: bytes of one workgroup's span (16 per thread)

struct LoaderArgs {
    const unsigned char* src;     // [n][H][W][C]
    const void* labels_src;       // [n] uint8 or int64
    unsigned long long* cursor;   // word 0: the step; the low half of word 1: the arrival counter
    int64_t* index;               // [batch]
    int64_t* labels;              // [batch]
    void* img;                    // float [batch][C][H][W] / uint8 [batch][H][W][C] / unused
    const float* mean;
    const float* inv_std;
    uint64_t seed;
    LdrGeom g;
    int hw, bytes, label_i64;     // H W; H W C
    unsigned spans, groups;       // workgroups per image; workgroups of the launch
};

// read-then-arrive on the cursor block: the protocol of spv_loader_core.h (shared with the fused fetch of spv_augment.hip)
__device__ __forceinline__ uint64_t read_step_and_arrive(const LoaderArgs& a) {
    const uint64_t t = ldr_read_step(a.cursor);
    ldr_arrive(a.cursor, t, a.groups);
    return t;
}

// sample b of step t: its row of the set (< n by construction: spv_loader_core.h); `record` writes the batch's index and label
__device__ __forceinline__ uint32_t fetch_sample(const LoaderArgs& a, uint64_t t, uint32_t b, bool record) {
    const uint32_t idx = ldr_index(a.seed, t, b, a.g);
    if (record) {
        a.index[b] = (int64_t)idx;
        a.labels[b] = a.label_i64 ? static_cast<const int64_t*>(a.labels_src)[idx]
                                  : (int64_t) static_cast<const unsigned char*>(a.labels_src)[idx];
    }
    return idx;
}

// mode none: one thread per sample
__global__ __launch_bounds__(LT) void loader_index_kernel(LoaderArgs a) {
    __shared__ uint64_t t_sh;
    if (threadIdx.x == 0) t_sh = read_step_and_arrive(a);
    __syncthreads();
    const uint32_t b = blockIdx.x * LT + threadIdx.x;
    if (b < a.g.batch) fetch_sample(a, t_sh, b, true);
}

// the workgroup's image and span: thread 0 reads the step and works the sample out, span 0 of an image records it
__device__ __forceinline__ void open_span(const LoaderArgs& a, uint32_t& b, uint32_t& span, uint32_t& idx) {
    __shared__ uint32_t idx_sh;
    b = blockIdx.x / a.spans;
    span = blockIdx.x - b * a.spans;
    if (threadIdx.x == 0) idx_sh = fetch_sample(a, read_step_and_arrive(a), b, span == 0);
    __syncthreads();
    idx = idx_sh;
}

// mode uint8: the image's H W C bytes copied unchanged, LDR_SPAN_BYTES per workgroup.  VEC: 16 bytes per thread.
template <bool VEC>
__global__ __launch_bounds__(LT) void loader_u8_kernel(LoaderArgs a) {
    uint32_t b, span, idx;
    open_span(a, b, span, idx);
    const size_t bytes = (size_t)a.bytes;
    const unsigned char* s = a.src + (size_t)idx * bytes;
    unsigned char* o = static_cast<unsigned char*>(a.img) + (size_t)b * bytes;
    const size_t lo = (size_t)span * LDR_SPAN_BYTES;
    if constexpr (VEC) {
        const size_t off = lo + (size_t)threadIdx.x * 16;
        if (off < bytes) *reinterpret_cast<uint4*>(o + off) = *reinterpret_cast<const uint4*>(s + off);   // bytes % 16 == 0
    } else {
        const size_t hi = lo + LDR_SPAN_BYTES < bytes ? lo + LDR_SPAN_BYTES : bytes;
        for (size_t off = lo + threadIdx.x; off < hi; off += LT) o[off] = s[off];
    }
}

__device__ __forceinline__ float normalise(unsigned v, float mean, float inv_std) { return ((float)v / 255.0f - mean) * inv_std; }

// mode float: NHWC bytes in, normalised planar fp32 out, LDR_SPAN_PX pixels per workgroup.  The span's bytes are staged in LDS as they
// lie in memory (coalesced reads); every thread then takes four neighbouring pixels of each channel from there -- C dwords at a
// stride of C dwords per thread, conflict-free for C = 1 and 3 -- and a wave writes 1 KiB of one plane per store instruction.
// VEC: 16-byte loads and stores.  Otherwise bytes in, single floats out, any size and alignment.
template <int C, bool VEC>
__global__ __launch_bounds__(LT) void loader_float_kernel(LoaderArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[LDR_SPAN_PX * C];
    uint32_t b, span, idx;
    open_span(a, b, span, idx);
    const int p0 = (int)span * LDR_SPAN_PX;
    const int npx = a.hw - p0 < LDR_SPAN_PX ? a.hw - p0 : LDR_SPAN_PX;
    const unsigned char* s = a.src + ((size_t)idx * a.hw + p0) * C;
    float* o = static_cast<float*>(a.img) + (size_t)b * C * a.hw + p0;
    const int tid = threadIdx.x;
    float mean[C], inv_std[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        mean[c] = a.mean[c];
        inv_std[c] = a.inv_std[c];
    }
    if constexpr (VEC) {
        // npx % 4 == 0 and npx C % 16 == 0: every 16-byte piece and every float4 lies wholly inside the image
        for (int k = tid; k * 16 < npx * C; k += LT)
            *reinterpret_cast<uint4*>(stage + k * 16) = *reinterpret_cast<const uint4*>(s + (size_t)k * 16);
        __syncthreads();
        if (4 * tid < npx) {
            unsigned w[C];
#pragma unroll
            for (int c = 0; c < C; ++c) w[c] = *reinterpret_cast<const unsigned*>(stage + (4 * tid * C) + 4 * c);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int at = j * C + c;   // byte of the thread's 4 C bytes
                    v[j] = normalise((w[at >> 2] >> (8 * (at & 3))) & 0xffu, mean[c], inv_std[c]);
                }
                *reinterpret_cast<float4*>(o + (size_t)c * a.hw + 4 * tid) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    } else {
        for (int k = tid; k < npx * C; k += LT) stage[k] = s[k];
        __syncthreads();
        for (int p = tid; p < npx; p += LT) {
#pragma unroll
            for (int c = 0; c < C; ++c) o[(size_t)c * a.hw + p] = normalise(stage[p * C + c], mean[c], inv_std[c]);
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

// the checks every fetch shares (spv_loader_fetch here, spv_loader_fetch_augment in spv_augment.hip), on the host before any launch
int spv_loader_check(const char* name, const unsigned char* src_nhwc, const void* labels_src, const void* cursor, const int64_t* index,
                     const int64_t* labels, const void* img, const float* mean, const float* inv_std, int n, int batch, int chans,
                     int height, int width, int world, int rank, int steps_per_epoch, int mode, int label_dtype) {
    SPV_CHECK(mode == SPV_LOADER_NONE || mode == SPV_LOADER_FLOAT || mode == SPV_LOADER_UINT8, "%s: unknown mode %d", name, mode);
    SPV_CHECK(label_dtype == SPV_LOADER_LABEL_U8 || label_dtype == SPV_LOADER_LABEL_I64, "%s: unknown label dtype %d", name,
              label_dtype);
    SPV_CHECK(labels_src && cursor && index && labels, "%s: null labels_src / cursor / index / labels", name);
    SPV_CHECK((reinterpret_cast<uintptr_t>(cursor) & 7u) == 0, "%s: cursor block not 8-byte aligned", name);
    SPV_CHECK(mode == SPV_LOADER_NONE || (src_nhwc && img), "%s: null src_nhwc / img in an image mode", name);
    SPV_CHECK(mode != SPV_LOADER_FLOAT || (mean && inv_std), "%s: mode float needs mean and inv_std", name);
    SPV_CHECK(n >= 1, "%s: n = %d samples (1 .. 2^31 - 1)", name, n);
    SPV_CHECK(batch >= 1, "%s: batch = %d must be positive", name, batch);
    SPV_CHECK(world >= 1 && rank >= 0 && rank < world, "%s: rank %d outside [0, world = %d)", name, rank, world);
    SPV_CHECK(steps_per_epoch >= 1 && (int64_t)steps_per_epoch * batch * world <= (int64_t)n,
              "%s: steps_per_epoch = %d: need 1 <= steps and steps * batch * world <= n (%d * %d * %d vs %d)", name, steps_per_epoch,
              steps_per_epoch, batch, world, n);
    SPV_CHECK((chans == 1 || chans == 3) && height >= 1 && height <= 512 && width >= 1 && width <= 512,
              "%s: chans = %d (1 or 3), height = %d, width = %d (1 .. 512)", name, chans, height, width);
    return 0;
}

extern "C" int64_t spv_loader_cursor_bytes() { return SPV_LOADER_CURSOR_BYTES; }

extern "C" int spv_loader_fetch(const unsigned char* src_nhwc, const void* labels_src, void* cursor, int64_t* index, int64_t* labels,
                                void* img, const float* mean, const float* inv_std, int n, int batch, int chans, int height, int width,
                                int world, int rank, int steps_per_epoch, uint64_t seed, int shuffle, int mode, int label_dtype,
                                void* stream) {
    if (int rc = spv_loader_check("spv_loader_fetch", src_nhwc, labels_src, cursor, index, labels, img, mean, inv_std, n, batch, chans, height,
                                  width, world, rank, steps_per_epoch, mode, label_dtype))
        return rc;
    LoaderArgs a;
    a.src = src_nhwc;
    a.labels_src = labels_src;
    a.cursor = static_cast<unsigned long long*>(cursor);
    a.index = index;
    a.labels = labels;
    a.img = img;
    a.mean = mean;
    a.inv_std = inv_std;
    a.seed = seed;
    a.g = LdrGeom{(uint32_t)n, (uint32_t)batch, (uint32_t)world, (uint32_t)rank, (uint32_t)steps_per_epoch, shuffle != 0};
    a.hw = height * width;
    a.label_i64 = label_dtype == SPV_LOADER_LABEL_I64;
    a.bytes = a.hw * chans;
    const int64_t bytes = a.bytes;
    a.spans = mode == SPV_LOADER_NONE ? 1u : (unsigned)(mode == SPV_LOADER_FLOAT ? cdiv(a.hw, LDR_SPAN_PX) : cdiv(bytes, LDR_SPAN_BYTES));
    const int64_t groups = mode == SPV_LOADER_NONE ? (int64_t)cdiv(batch, LT) : (int64_t)batch * a.spans;
    SPV_CHECK(groups < (1ll << 31), "spv_loader_fetch: batch = %d of %d x %d x %d images needs %lld workgroups (< 2^31)", batch, chans,
              height, width, (long long)groups);
    a.groups = (unsigned)groups;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)groups), block(LT);
    if (mode == SPV_LOADER_NONE) {
        loader_index_kernel<<<grid, block, 0, st>>>(a);
    } else if (mode == SPV_LOADER_UINT8) {
        const bool vec = bytes % 16 == 0 && aligned16(src_nhwc) && aligned16(img);
        if (vec) loader_u8_kernel<true><<<grid, block, 0, st>>>(a);
        else loader_u8_kernel<false><<<grid, block, 0, st>>>(a);
    } else {
        const bool vec = bytes % 16 == 0 && a.hw % 4 == 0 && aligned16(src_nhwc) && aligned16(img);
        if (chans == 3) {
            if (vec) loader_float_kernel<3, true><<<grid, block, 0, st>>>(a);
            else loader_float_kernel<3, false><<<grid, block, 0, st>>>(a);
        } else {
            if (vec) loader_float_kernel<1, true><<<grid, block, 0, st>>>(a);
            else loader_float_kernel<1, false><<<grid, block, 0, st>>>(a);
        }
    }
    SPV_LAUNCH_CHECK("spv_loader_fetch");
    return 0;
}
