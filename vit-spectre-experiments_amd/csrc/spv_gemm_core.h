// The host side of spv_gemm.hip's dispatch: the strip kernel's share plan and three pure selectors that name, for one call of an
// entry family (spv_gemm_nt*, spv_gemm_tn / _fold, spv_gemm_tn_batch / _part), either the refusal or the ONE kernel that serves it,
// with its grid and the reduce that follows.  launch_gemm, gemm_tn_impl and gemm_tn_batch_impl switch on the answer and do nothing
// else to choose.  No HIP type in it: tests/test_gemm_ref.py compiles it with a plain C++ compiler and holds every selector to the
// Python restatement tests/gemm_edge_cases.py over a grid that straddles each threshold.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int GEMM_BM = 128, GEMM_BN = 128;   // the 128 x 128 tile of the NT tile / direct-to-LDS kernels and of the TN tile kernel
constexpr int GEMM_GBK = 64;                  // split-K slices of the direct-to-LDS kernel are multiples of this many bf16 elements
constexpr int GEMM_TBK = 64;                  // k rows per stage of the TN kernels
constexpr int GEMM_TWM = 256;                 // rows of the wide TN tile
constexpr int GEMM_TTM = 512, GEMM_TTK = 32;  // the tall TN kernel: all of M = 512 in one workgroup, 32 k rows per stage
constexpr int GEMM_TNB_MAX = 8;               // problems of one batched TN launch
constexpr int GEMM_FJ_MAX = 16;               // fold jobs of one launch
constexpr int GEMM_FOLD_THREADS = 1024;       // FOLD_COLS * FOLD_ROWS (spv_common.h)
constexpr int GEMM_DT_F32 = 0, GEMM_DT_BF16 = 1;   // SPV_F32, SPV_BF16

inline int gemm_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// workgroups of a split-K sum: `threads` per workgroup, four columns per thread when N % 4 == 0, at most 2048
inline int gemm_reduce_blocks(int M, int N, int threads) {
    const int64_t b = ((int64_t)M * N / ((N & 3) == 0 ? 4 : 1) + threads - 1) / threads;
    return (int)(b < 2048 ? b : 2048);
}

// the uneven shares of the strip kernel: `groups` row groups of base (+1 for the first rem) 32-row blocks; picks the
// wave-row height MB whose sub-tiles (2 MB or 2 MB + 1 blocks) cover base and base + 1 without padding.
// reserved_cus: CUs the strip kernel leaves alone (spv_set_reserved_cus): a strip workgroup needs a whole CU (2 x 256 VGPRs per SIMD,
// 155 KiB of LDS), so on a CU that holds a resident RCCL channel it cannot start and would run as a second dispatch round.  16
// reserved CUs cost nothing at the layer shapes (the largest share stays 9 / 13 row blocks).
inline bool strip_plan(int M, int N, int K, int reserved_cus, int& MB, int& nstrips, int& groups, int& base, int& rem) {
    if (N <= 0 || N % 256 != 0 || N > 16384 || K % 128 != 0 || K < 128 || M < 8192) return false;   // (Base width: the MHPermutMix data gradient has N = 9216)
    nstrips = N / 256;
    const int nblk = gemm_cdiv(M, 32);
    groups = (256 - reserved_cus) / nstrips;
    if (groups < 1) return false;
    if (groups > nblk) groups = nblk;
    base = nblk / groups;
    rem = nblk % groups;
    auto padded = [&](int mb, int c) {  // MFMA block slots a run of c blocks occupies
        int slots = 0;
        while (c > 0) {
            const int full = 2 * mb;
            const int take = (c % full != 0 && c >= full + 1) ? full + 1 : (full < c ? full : c);
            slots += take >= full ? take : full;
            c -= take;
        }
        return slots;
    };
    int best = 0, best_slots = 1 << 30;
    const int worst = base + (rem ? 1 : 0);
    for (int mb = 4; mb >= 2; --mb) {
        const int s = padded(mb, worst);
        if (s < best_slots) { best_slots = s; best = mb; }
    }
    if (best == 0 || best_slots * 100 > worst * 115) return false;  // more than 15 % padding: the 128 x 128 kernels do better
    MB = best;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------------ NT
enum GemmNtKernel : int {
    GEMM_NT_REFUSE_EMPTY = 0,    // M, N or K <= 0
    GEMM_NT_REFUSE_DTYPE,        // in / out dtype neither SPV_F32 nor SPV_BF16
    GEMM_NT_REFUSE_CHUNK,        // K, lda or ldb not a multiple of 16 bytes of input elements
    GEMM_NT_REFUSE_ALIGN,        // A or B not 16-byte aligned
    GEMM_NT_REFUSE_LD,           // lda < K, ldb < K or ldc < N
    GEMM_NT_REFUSE_SPLITS,       // splits < 1
    GEMM_NT_REFUSE_WORKSPACE,    // splits > 1 without a workspace, or with one that is not 16-byte aligned (16-byte slab stores)
    GEMM_NT_ROWS,                // gemm_nt_rows_kernel<TO>
    GEMM_NT_STRIP,               // gemm_nt_strip_kernel<mb, epi>
    GEMM_NT_GLDS,                // gemm_nt_glds_kernel<TO, 128, 2>
    GEMM_NT_TILE,                // gemm_nt_kernel<T, TO>
    GEMM_NT_KERNEL_COUNT
};
inline const char* gemm_nt_kernel_name(int k) {
    static const char* const names[GEMM_NT_KERNEL_COUNT] = {"refuse_empty", "refuse_dtype", "refuse_chunk", "refuse_align", "refuse_ld", "refuse_splits",
                                                            "refuse_workspace", "rows", "strip", "glds", "tile"};
    return k >= 0 && k < GEMM_NT_KERNEL_COUNT ? names[k] : "?";
}

// *_lo: the low four bits of that pointer; -1: the pointer is NULL (bias, bias2d, workspace)
struct GemmNtCall {
    int in_dtype, out_dtype, M, N, K, lda, ldb, ldc;
    int a_lo, b_lo, c_lo, bias_lo;
    int accumulate, splits, ws_lo;
    int rg, bias2d_lo;               // grouped output rows (rg > 0) and their 2-D bias
    int pool, pool_pw, pool_bf16;    // the pool-backward operand: present, its window, stored as bf16
    int drop;                        // p_drop > 0
    int reserved_cus;
};
struct GemmNtPlan {
    GemmNtKernel kernel;
    int splits, k_per_split;         // as recomputed: slices of whole K-tiles, no empty slice
    int grid;                        // workgroups of the GEMM launch
    int mb, epi, nstrips, groups, base, rem;   // strip only; epi 0 store, 1 accumulate, 2 pool in one window, 3 pool across two windows
    int reduce;                      // 1: splitk_reduce_kernel<TO> follows
    int reduce_blocks;
};

inline GemmNtPlan gemm_nt_plan(const GemmNtCall& c) {
    GemmNtPlan p{};
    auto refuse = [&](GemmNtKernel k) { p.kernel = k; return p; };
    if (!(c.M > 0 && c.N > 0 && c.K > 0)) return refuse(GEMM_NT_REFUSE_EMPTY);
    if ((c.in_dtype != GEMM_DT_F32 && c.in_dtype != GEMM_DT_BF16) || (c.out_dtype != GEMM_DT_F32 && c.out_dtype != GEMM_DT_BF16))
        return refuse(GEMM_NT_REFUSE_DTYPE);
    const bool in_bf = c.in_dtype == GEMM_DT_BF16, out_bf = c.out_dtype == GEMM_DT_BF16;
    const int ch = in_bf ? 8 : 4;
    if (!(c.K % ch == 0 && c.lda % ch == 0 && c.ldb % ch == 0)) return refuse(GEMM_NT_REFUSE_CHUNK);
    if (!(c.a_lo == 0 && c.b_lo == 0)) return refuse(GEMM_NT_REFUSE_ALIGN);
    if (!(c.lda >= c.K && c.ldb >= c.K && c.ldc >= c.N)) return refuse(GEMM_NT_REFUSE_LD);
    if (c.splits < 1) return refuse(GEMM_NT_REFUSE_SPLITS);
    if (c.splits > 1 && c.ws_lo != 0) return refuse(GEMM_NT_REFUSE_WORKSPACE);
    const int BK = in_bf ? 64 : 32;   // elements in the 128 bytes of K of one tile row
    const int tiles_m = gemm_cdiv(c.M, GEMM_BM), tiles_n = gemm_cdiv(c.N, GEMM_BN);
    p.splits = 1;
    p.k_per_split = c.K;
    if (c.splits > 1) {
        p.k_per_split = gemm_cdiv(gemm_cdiv(c.K, c.splits), BK) * BK;
        p.splits = gemm_cdiv(c.K, p.k_per_split);
    }
    p.grid = tiles_m * tiles_n * p.splits;
    p.reduce = p.splits > 1;
    p.reduce_blocks = p.reduce ? gemm_reduce_blocks(c.M, c.N, 256) : 0;
    const bool plain = c.rg == 0 && c.bias2d_lo < 0 && !c.drop;
    // few rows: one 32 x 32 tile per workgroup straight from the L2-resident operands (no split-K workspace, no reduce launch)
    // (K <= 1536: a wave walks its K share in batches of 8 k-steps, one L2 round trip each -- at K = 8192 that chain is 40 us against
    // 15 + 5 for split-K + reduce; <= 1024 tiles: beyond that the 32 x 32 tiles re-read the operands 4x as often as 128 x 128 ones)
    const int t32 = gemm_cdiv(c.M, 32) * gemm_cdiv(c.N, 32);
    if (in_bf && p.splits == 1 && c.M <= 2048 && c.K <= 1536 && plain && !c.pool && c.K % 16 == 0 && t32 >= 64 && t32 <= 1024) {
        p.kernel = GEMM_NT_ROWS;
        p.grid = t32;
        return p;
    }
    if (in_bf && out_bf) {
        const bool pool_ok = !c.pool || (c.pool_bf16 && !c.accumulate && c.pool_pw >= 8 && c.N % c.pool_pw == 0);   // (8 columns span <= 2 windows)
        const bool span32 = (uint64_t)c.M * c.lda * 2 < (1ull << 32) && (uint64_t)c.N * c.ldb * 2 < (1ull << 32);    // 32-bit DMA source offsets
        if (p.splits == 1 && plain && pool_ok && span32 && c.ldc % 8 == 0 && c.c_lo == 0 && (c.bias_lo < 0 || (c.bias_lo & 3) == 0) &&
            strip_plan(c.M, c.N, c.K, c.reserved_cus, p.mb, p.nstrips, p.groups, p.base, p.rem)) {
            p.kernel = GEMM_NT_STRIP;
            p.epi = c.pool ? (c.pool_pw % 8 != 0 ? 3 : 2) : c.accumulate ? 1 : 0;   // the two-window epilogue is its own instantiation (in the one-window kernel it cost 6 %)
            p.grid = p.groups * p.nstrips;
            return p;
        }
        p.mb = p.nstrips = p.groups = p.base = p.rem = 0;
    }
    // direct-to-LDS double-buffered kernel for long reductions (measured: 896 vs 795 TFLOP/s at 4096^3, 755 vs 700 on
    // the 512 x 8192 x 33280 weight gradient); the skinny K <= 1024 layer GEMMs are faster on the register-staged
    // kernel (42 vs 50 us at 33280 x 768 x 512: three workgroups per CU instead of two)
    // K <= 1024 (the layer GEMMs) stays on the register-staged kernel: the three-stage 64-byte-row ring measures the
    // same step time (2.978 vs 2.972 ms over three alternating runs) and 4 us more per isolated launch
    const int slice = c.K < p.k_per_split ? c.K : p.k_per_split;
    p.kernel = in_bf && c.K % GEMM_GBK == 0 && p.k_per_split % GEMM_GBK == 0 && slice > 1024 ? GEMM_NT_GLDS : GEMM_NT_TILE;
    return p;
}

// ------------------------------------------------------------------------------------------------------------------------ TN
enum GemmTnKernel : int {
    GEMM_TN_REFUSE_EMPTY = 0,    // M, N or K <= 0
    GEMM_TN_REFUSE_DTYPE,        // out dtype neither SPV_F32 nor SPV_BF16
    GEMM_TN_REFUSE_CHUNK,        // M, N, lda or ldb not a multiple of 8
    GEMM_TN_REFUSE_ALIGN,        // A or B not 16-byte aligned
    GEMM_TN_REFUSE_LD,           // lda < M, ldb < N or ldc < N
    GEMM_TN_REFUSE_WORKSPACE,    // splits < 1, or splits > 1 without a 16-byte aligned workspace
    GEMM_TN_REFUSE_FOLDS,        // more than 16 fold jobs, or a bad one
    GEMM_TN_TALL,                // gemm_tn_tall_kernel<TO>
    GEMM_TN_WIDE,                // gemm_tn_wide_kernel<TO>
    GEMM_TN_TILE1,               // gemm_tn_kernel<TO, 1>
    GEMM_TN_TILE3,               // gemm_tn_kernel<TO, 3>
    GEMM_TN_KERNEL_COUNT
};
inline const char* gemm_tn_kernel_name(int k) {
    static const char* const names[GEMM_TN_KERNEL_COUNT] = {"refuse_empty", "refuse_dtype", "refuse_chunk", "refuse_align", "refuse_ld", "refuse_workspace",
                                                            "refuse_folds", "tall", "wide", "tile1", "tile3"};
    return k >= 0 && k < GEMM_TN_KERNEL_COUNT ? names[k] : "?";
}
enum GemmTnReduce : int {
    GEMM_TN_NO_REDUCE = 0,       // one slab, no folds: the GEMM stored C
    GEMM_TN_REDUCE_PLAIN,        // splitk_reduce_kernel<TO>
    GEMM_TN_REDUCE_FOLDS,        // splitk_reduce_fold_kernel<TO>: the folds ride as extra workgroups
    GEMM_TN_FOLD_ALONE           // one slab: fold_multi_kernel by itself
};
struct GemmTnPlan {
    GemmTnKernel kernel;
    GemmTnReduce reduce;
    int splits, k_per_split;
    int grid;                    // workgroups of the GEMM launch
    int reduce_blocks;           // summing workgroups of the reduce (the fold workgroups come on top)
};
// fold_blocks: workgroups the call's fold jobs need (0: none, -1: a bad job or too many)
inline GemmTnPlan gemm_tn_plan(int out_dtype, int M, int N, int K, int lda, int ldb, int ldc, int a_lo, int b_lo, int splits, int ws_lo, int fold_blocks) {
    GemmTnPlan p{};
    auto refuse = [&](GemmTnKernel k) { p.kernel = k; return p; };
    if (!(M > 0 && N > 0 && K > 0)) return refuse(GEMM_TN_REFUSE_EMPTY);
    if (out_dtype != GEMM_DT_F32 && out_dtype != GEMM_DT_BF16) return refuse(GEMM_TN_REFUSE_DTYPE);
    if (!(M % 8 == 0 && N % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0)) return refuse(GEMM_TN_REFUSE_CHUNK);
    if (!(a_lo == 0 && b_lo == 0)) return refuse(GEMM_TN_REFUSE_ALIGN);
    if (!(lda >= M && ldb >= N && ldc >= N)) return refuse(GEMM_TN_REFUSE_LD);
    if (!(splits >= 1 && (splits == 1 || ws_lo == 0))) return refuse(GEMM_TN_REFUSE_WORKSPACE);
    if (fold_blocks < 0) return refuse(GEMM_TN_REFUSE_FOLDS);
    const int tiles_m = gemm_cdiv(M, GEMM_BM), tiles_n = gemm_cdiv(N, GEMM_BN);
    p.splits = 1;
    p.k_per_split = K;
    if (splits > 1) {
        p.k_per_split = gemm_cdiv(gemm_cdiv(K, splits), GEMM_TBK) * GEMM_TBK;
        p.splits = gemm_cdiv(K, p.k_per_split);
    }
    constexpr int wide_min = 4;   // fewest split-K slabs that pay for the 256 x 128 tile
    if (M == GEMM_TTM && N % GEMM_BN == 0 && N >= 8 * GEMM_BN && tiles_n * p.splits >= 192 && p.k_per_split >= 16 * GEMM_TTK) {
        // all of M in one workgroup: the B panel (the gathered matrix of the MHPermutMix gradient) is read once
        p.kernel = GEMM_TN_TALL;
        p.grid = tiles_n * p.splits;
    } else if (p.splits >= wide_min && M % GEMM_TWM == 0 && N % GEMM_BN == 0 && (M / GEMM_TWM) * tiles_n * p.splits >= 128) {
        // the 256 x 128 tile (8 waves, one workgroup per CU): the split-K layer weight gradients.  Measured in graph mode, alternating,
        // against the 128 x 128 kernel: 2.372 vs 2.385 ms/step -- 1.6 us per launch; without split-K (the MHPermutMix weight gradient,
        // 512 x 8192 x 33 280) it is SLOWER (651 vs 510 us), hence splits >= 4
        p.kernel = GEMM_TN_WIDE;
        p.grid = (M / GEMM_TWM) * tiles_n * p.splits;
    } else {
        // One K-tile in flight (144 VGPRs, 40 KB of LDS) for the sliver-shaped gradient of the patch embedding (512 x 48 x 33 280): that
        // launch runs on the main stream BESIDE the batched layer gradients, whose workgroups (8 waves x 184 VGPRs, 112 KB) leave exactly
        // 144 VGPRs per SIMD and 45 KB per CU -- with three tiles in flight (216 VGPRs) its workgroups waited for those CUs to drain.
        p.kernel = N <= 64 ? GEMM_TN_TILE1 : GEMM_TN_TILE3;
        p.grid = tiles_m * tiles_n * p.splits;
    }
    p.reduce = p.splits > 1 ? (fold_blocks > 0 ? GEMM_TN_REDUCE_FOLDS : GEMM_TN_REDUCE_PLAIN) : (fold_blocks > 0 ? GEMM_TN_FOLD_ALONE : GEMM_TN_NO_REDUCE);
    p.reduce_blocks = p.splits > 1 ? gemm_reduce_blocks(M, N, 256) : 0;
    return p;
}

// ------------------------------------------------------------------------------------------------------------------ TN batch
enum GemmTnBatchKernel : int {
    GEMM_TNB_REFUSE_COUNT = 0,   // no problems, or more than 8
    GEMM_TNB_REFUSE_CALL,        // K <= 0, splits < 1, or no 16-byte aligned workspace
    GEMM_TNB_REFUSE_FOLDS,       // more than 16 fold jobs, or a bad one
    GEMM_TNB_REFUSE_K,           // a problem's k outside 0..K
    GEMM_TNB_REFUSE_NO_LONG,     // no problem reduces over the call's K rows
    GEMM_TNB_REFUSE_EMPTY,       // a problem with a NULL pointer or m, n <= 0
    GEMM_TNB_REFUSE_SHAPE,       // m, n, lda, ldb not multiples of 8, or a leading dimension below its extent
    GEMM_TNB_REFUSE_ALIGN,       // a problem's A or B not 16-byte aligned
    GEMM_TNB_REFUSE_SHORT_LDC,   // a short problem whose ldc is not a multiple of 4
    GEMM_TNB_128,                // gemm_tn_batch_kernel<3>
    GEMM_TNB_WIDE,               // gemm_tn_batch_wide_kernel
    GEMM_TNB_KERNEL_COUNT
};
inline const char* gemm_tnb_kernel_name(int k) {
    static const char* const names[GEMM_TNB_KERNEL_COUNT] = {"refuse_count", "refuse_call", "refuse_folds", "refuse_k", "refuse_no_long", "refuse_empty",
                                                             "refuse_shape", "refuse_align", "refuse_short_ldc", "batch128", "batch_wide"};
    return k >= 0 && k < GEMM_TNB_KERNEL_COUNT ? names[k] : "?";
}
struct GemmTnBatchProblem {
    int m, n, lda, ldb, ldc, k;
    int a_lo, b_lo;              // the low four bits of a and b
    int has_ptrs;                // a, b and c are all non-NULL
};
struct GemmTnBatchPlan {
    GemmTnBatchKernel kernel;
    int bad;                             // the caller's index of the problem a refusal is about (-1: the call itself)
    int splits, k_per_split;
    int nlong;                           // problems [0, nlong) of order[] reduce over the call's K rows in `splits` slices; the rest over their own first k rows, unsplit
    int order[GEMM_TNB_MAX];             // kernel problem index -> the caller's: long problems first, each kind in the caller's order
    int first_tile[GEMM_TNB_MAX + 1];    // 128 x 128 tiles in front of each problem (the 128 form)
    int wide_first_tile[GEMM_TNB_MAX + 1];   // 256 x 128 tiles in front of each problem (the wide form)
    long long ws_off[GEMM_TNB_MAX];      // floats into the workspace: `splits` slabs of m x n per LONG problem, problem after problem
    int grid;                            // workgroups of the GEMM launch: the long tiles of every slice + the short tiles padded to a multiple of 8
    int reduce_blocks;                   // summing workgroups per long problem in the reduce launch
};
inline GemmTnBatchPlan gemm_tn_batch_plan(const GemmTnBatchProblem* q, int nprob, int K, int splits, int ws_lo, int fold_blocks) {
    GemmTnBatchPlan p{};
    p.bad = -1;
    auto refuse = [&](GemmTnBatchKernel k, int which) { p.kernel = k; p.bad = which; return p; };
    if (!(q != nullptr && nprob >= 1 && nprob <= GEMM_TNB_MAX)) return refuse(GEMM_TNB_REFUSE_COUNT, -1);
    if (!(K > 0 && splits >= 1 && ws_lo == 0)) return refuse(GEMM_TNB_REFUSE_CALL, -1);
    if (fold_blocks < 0) return refuse(GEMM_TNB_REFUSE_FOLDS, -1);
    p.k_per_split = gemm_cdiv(gemm_cdiv(K, splits), GEMM_TBK) * GEMM_TBK;
    p.splits = gemm_cdiv(K, p.k_per_split);
    int no = 0;
    for (int i = 0; i < nprob; ++i) {
        if (!(q[i].k >= 0 && q[i].k <= K)) return refuse(GEMM_TNB_REFUSE_K, i);
        if (q[i].k == 0 || q[i].k == K) p.order[no++] = i;
    }
    p.nlong = no;
    for (int i = 0; i < nprob; ++i)
        if (!(q[i].k == 0 || q[i].k == K)) p.order[no++] = i;
    if (p.nlong < 1) return refuse(GEMM_TNB_REFUSE_NO_LONG, -1);
    int tiles = 0, wt = 0, long_tiles = 0, wlong = 0;
    long long off = 0;
    p.reduce_blocks = 1;
    // the 256 x 128 tile when every problem divides into it and the K-slices are long enough to pay for its longer prologue
    bool wide = p.k_per_split >= 8 * GEMM_TBK;
    for (int i = 0; i < nprob; ++i) {
        const GemmTnBatchProblem& r = q[p.order[i]];
        if (!(r.has_ptrs && r.m > 0 && r.n > 0)) return refuse(GEMM_TNB_REFUSE_EMPTY, p.order[i]);
        if (!(r.m % 8 == 0 && r.n % 8 == 0 && r.lda % 8 == 0 && r.ldb % 8 == 0 && r.lda >= r.m && r.ldb >= r.n && r.ldc >= r.n))
            return refuse(GEMM_TNB_REFUSE_SHAPE, p.order[i]);
        if (!(r.a_lo == 0 && r.b_lo == 0)) return refuse(GEMM_TNB_REFUSE_ALIGN, p.order[i]);
        if (!(i < p.nlong || r.ldc % 4 == 0)) return refuse(GEMM_TNB_REFUSE_SHORT_LDC, p.order[i]);
        wide = wide && r.m % GEMM_TWM == 0 && r.n % GEMM_BN == 0 && (r.k == 0 || r.k >= GEMM_TBK);
        p.first_tile[i] = tiles;
        p.wide_first_tile[i] = wt;
        p.ws_off[i] = off;
        tiles += gemm_cdiv(r.m, GEMM_BM) * gemm_cdiv(r.n, GEMM_BN);
        wt += (r.m / GEMM_TWM) * gemm_cdiv(r.n, GEMM_BN);
        if (i < p.nlong) {
            long_tiles = tiles;
            wlong = wt;
            off += (long long)p.splits * r.m * r.n;
            const int rb = gemm_reduce_blocks(r.m, r.n, GEMM_FOLD_THREADS);
            if (rb > p.reduce_blocks) p.reduce_blocks = rb;
        }
    }
    p.first_tile[nprob] = tiles;
    p.wide_first_tile[nprob] = wt;
    p.kernel = wide ? GEMM_TNB_WIDE : GEMM_TNB_128;
    p.grid = wide ? wlong * p.splits + ((wt - wlong + 7) & ~7) : long_tiles * p.splits + ((tiles - long_tiles + 7) & ~7);
    return p;
}
