// spv_snapshot_multi (include/spv.h): a run's device-resident state copied, bit for bit, into the slots of one
// flat staging buffer by ONE launch over a chunk table -- the table shape of spv_adamw_multi, with bytes where that one has elements.
// Each chunk also leaves two partials at a fixed place: the sum of its 32-bit words (the file's checksum, folded on the host) and,
// for fp32 jobs, its count of values with an all-ones exponent (the gate that keeps a diverged run from replacing a checkpoint).
// Plain vector loads and stores, no atomics, nothing allocated and nothing synchronised: the launch may be captured.
#include "spv_common.h"

namespace {

constexpr int SNAP_THREADS = 256;
constexpr int SNAP_UNROLL = 4;   // 16-byte loads a lane has in flight: 256 lanes x 4 x 16 B = 16 KiB per workgroup and round

__device__ __forceinline__ int nonfinite32(unsigned w) { return (w & 0x7f800000u) == 0x7f800000u; }

// bytes [begin, end) of the chunk one at a time; `begin` is a multiple of 4 from the job's start, so byte i sits in lane i & 3 of its
// little-endian word and a job's last partial word counts as zero-padded.  Counted jobs: every WHOLE word of the range once more,
// put together from its bytes (the source need not be aligned).
__device__ __forceinline__ void snap_bytes(const unsigned char* src, unsigned char* dst, long long begin, long long end, int counted, int tid,
                                           unsigned long long& sum, int& bad) {
    for (long long i = begin + tid; i < end; i += SNAP_THREADS) {
        const unsigned char b = src[i];
        dst[i] = b;
        sum += (unsigned long long)b << (8 * (int)((i - begin) & 3));
    }
    if (counted) {
        for (long long w = begin + 4LL * tid; w + 4 <= end; w += 4LL * SNAP_THREADS)
            bad += nonfinite32((unsigned)src[w] | (unsigned)src[w + 1] << 8 | (unsigned)src[w + 2] << 16 | (unsigned)src[w + 3] << 24);
    }
}

__global__ __launch_bounds__(SNAP_THREADS) void snapshot_multi_kernel(const spv_copy_job* __restrict__ jobs, const int* __restrict__ chunk_job,
                                                                      const long long* __restrict__ chunk_off, int chunk_bytes,
                                                                      unsigned long long* __restrict__ chunk_sum,
                                                                      int* __restrict__ chunk_nonfinite) {
    const int c = blockIdx.x, tid = threadIdx.x;
    const spv_copy_job job = jobs[chunk_job[c]];
    const long long off = chunk_off[c];
    long long len = job.bytes - off;
    if (len > chunk_bytes) len = chunk_bytes;
    if (len < 0) len = 0;   // (a table row past its job's end copies nothing)
    const unsigned char* src = static_cast<const unsigned char*>(job.src) + off;
    unsigned char* dst = static_cast<unsigned char*>(job.dst) + off;
    const int counted = job.kind == 1;
    const unsigned long long both = (unsigned long long)(uintptr_t)src | (unsigned long long)(uintptr_t)dst;

    unsigned long long sum = 0;
    int bad = 0;
    long long done = 0;   // bytes the vector walk took; the rest goes bytewise
    if ((both & 15) == 0) {
        const long long n16 = len >> 4;
        const uint4* s = reinterpret_cast<const uint4*>(src);
        uint4* d = reinterpret_cast<uint4*>(dst);
        long long i = tid;
        for (; i + (SNAP_UNROLL - 1) * SNAP_THREADS < n16; i += SNAP_UNROLL * SNAP_THREADS) {
            uint4 v[SNAP_UNROLL];
#pragma unroll
            for (int u = 0; u < SNAP_UNROLL; ++u) v[u] = s[i + u * SNAP_THREADS];
#pragma unroll
            for (int u = 0; u < SNAP_UNROLL; ++u) {
                d[i + u * SNAP_THREADS] = v[u];
                sum += ((unsigned long long)v[u].x + v[u].y) + ((unsigned long long)v[u].z + v[u].w);
                if (counted) bad += nonfinite32(v[u].x) + nonfinite32(v[u].y) + nonfinite32(v[u].z) + nonfinite32(v[u].w);
            }
        }
        for (; i < n16; i += SNAP_THREADS) {
            const uint4 v = s[i];
            d[i] = v;
            sum += ((unsigned long long)v.x + v.y) + ((unsigned long long)v.z + v.w);
            if (counted) bad += nonfinite32(v.x) + nonfinite32(v.y) + nonfinite32(v.z) + nonfinite32(v.w);
        }
        done = n16 << 4;
    } else if ((both & 3) == 0) {
        const long long n4 = len >> 2;
        const unsigned* s = reinterpret_cast<const unsigned*>(src);
        unsigned* d = reinterpret_cast<unsigned*>(dst);
        long long i = tid;
        for (; i + (SNAP_UNROLL - 1) * SNAP_THREADS < n4; i += SNAP_UNROLL * SNAP_THREADS) {
            unsigned v[SNAP_UNROLL];
#pragma unroll
            for (int u = 0; u < SNAP_UNROLL; ++u) v[u] = s[i + u * SNAP_THREADS];
#pragma unroll
            for (int u = 0; u < SNAP_UNROLL; ++u) {
                d[i + u * SNAP_THREADS] = v[u];
                sum += v[u];
                if (counted) bad += nonfinite32(v[u]);
            }
        }
        for (; i < n4; i += SNAP_THREADS) {
            const unsigned v = s[i];
            d[i] = v;
            sum += v;
            if (counted) bad += nonfinite32(v);
        }
        done = n4 << 2;
    }
    snap_bytes(src, dst, done, len, counted, tid, sum, bad);

    // the workgroup's two partials, summed in a fixed tree (integer sums: the order could not change them, the layout is fixed anyway)
    __shared__ unsigned long long red_sum[SNAP_THREADS];
    __shared__ int red_bad[SNAP_THREADS];
    red_sum[tid] = sum;
    red_bad[tid] = bad;
    __syncthreads();
#pragma unroll
    for (int step = SNAP_THREADS / 2; step > 0; step >>= 1) {
        if (tid < step) {
            red_sum[tid] += red_sum[tid + step];
            red_bad[tid] += red_bad[tid + step];
        }
        __syncthreads();
    }
    if (tid == 0) {
        chunk_sum[c] = red_sum[0];
        chunk_nonfinite[c] = red_bad[0];
    }
}

}  // namespace

extern "C" int spv_snapshot_multi(const spv_copy_job* jobs, const int* chunk_job, const long long* chunk_off, int nchunks, int chunk_bytes,
                                  unsigned long long* chunk_sum, int* chunk_nonfinite, void* stream) {
    SPV_CHECK(nchunks >= 0, "spv_snapshot_multi: nchunks = %d", nchunks);
    SPV_CHECK(chunk_bytes > 0 && chunk_bytes % 16 == 0, "spv_snapshot_multi: chunk_bytes = %d must be a positive multiple of 16", chunk_bytes);
    if (nchunks == 0) return 0;
    SPV_CHECK(jobs && chunk_job && chunk_off, "spv_snapshot_multi: null table");
    SPV_CHECK(chunk_sum && chunk_nonfinite, "spv_snapshot_multi: null chunk_sum / chunk_nonfinite");
    hipLaunchKernelGGL(snapshot_multi_kernel, dim3(nchunks), dim3(SNAP_THREADS), 0, static_cast<hipStream_t>(stream), jobs, chunk_job,
                       chunk_off, chunk_bytes, chunk_sum, chunk_nonfinite);
    SPV_LAUNCH_CHECK("spv_snapshot_multi");
    return 0;
}
