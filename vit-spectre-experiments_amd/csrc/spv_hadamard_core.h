// The host side of spv_hadamard.hip's 2-D dispatch: one pure selector that names, for a call of spv_hadamard_mix, either the refusal
// or the ONE kernel plan that serves it, and the window rules of the fused and row-0 entry points.  The entry points switch on these
// answers and do nothing else to choose; spv_hadamard_path returns the selector's code.  No HIP type in it: it compiles with a plain
// C++ compiler, and tests/hadamard_ref.py restates it in Python.
#pragma once
#include <stddef.h>
#include <stdint.h>

// codes of spv_hadamard_path (include/spv.h names the same values)
constexpr int HADAMARD_ONE_KERNEL = 1;          // hadamard_lds_kernel<T>: the padded image in LDS as fp32
constexpr int HADAMARD_GENERIC = 2;             // hadamard_rows_kernel<T> -> fp32 workspace -> hadamard_cols_kernel<T>
constexpr int HADAMARD_REFUSE_EMPTY = -1;       // tokens < 1 or dim < 1
constexpr int HADAMARD_REFUSE_DTYPE = -2;       // neither SPV_F32 (0) nor SPV_BF16 (1)
constexpr int HADAMARD_REFUSE_DIM = -3;         // next_pow2(dim) > 16384
constexpr int HADAMARD_REFUSE_TOKENS = -4;      // generic path: next_pow2(tokens) > 32768 (one padded column no longer fits the slab)
constexpr int HADAMARD_REFUSE_WORKSPACE = -5;   // generic path without a workspace

constexpr int HADAMARD_MAX_DP = 16384;
constexpr int HADAMARD_MAX_NP = 32768;
constexpr int HADAMARD_ONE_MAX_TOKENS = 128;    // the one-kernel token pass is a direct +-1 sum, tokens^2 per column
constexpr size_t HADAMARD_LDS_LIMIT = 160 * 1024;
constexpr size_t HADAMARD_SLAB_LDS = 128 * 1024;   // the generic column slab: next_pow2(tokens) x cs floats
constexpr int HADAMARD_LN_DIM = 512, HADAMARD_LN_MIN_TOKENS = 2, HADAMARD_LN_MAX_TOKENS = 65;

inline int hadamard_next_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
inline int hadamard_log2(int p) {
    int l = 0;
    while ((1 << l) < p) ++l;
    return l;
}

struct HadamardPlan {
    int path;        // one of the codes above
    int np, dp;      // padded sizes (0 when refused before they are formed)
    int rpw;         // generic: rows per workgroup of the row pass
    int cs;          // generic: columns per slab of the column pass
    size_t lds;      // one-kernel: bytes of LDS; generic: of the larger of its two launches
};

inline HadamardPlan hadamard_select(int dtype, int tokens, int dim, bool has_workspace) {
    HadamardPlan p = {HADAMARD_REFUSE_EMPTY, 0, 0, 0, 0, 0};
    if (tokens < 1 || dim < 1) return p;
    if (dtype != 0 && dtype != 1) { p.path = HADAMARD_REFUSE_DTYPE; return p; }
    if (dim > HADAMARD_MAX_DP) { p.path = HADAMARD_REFUSE_DIM; return p; }
    p.dp = hadamard_next_pow2(dim);
    // one kernel: rows are whole 16-byte pieces in either dtype, and the fp32 image fits (the kernel has no scratch beside it)
    if (dim % 8 == 0 && tokens <= HADAMARD_ONE_MAX_TOKENS && (size_t)tokens * p.dp * 4 <= HADAMARD_LDS_LIMIT) {
        p.np = hadamard_next_pow2(tokens);
        p.lds = (size_t)tokens * p.dp * 4;
        p.path = HADAMARD_ONE_KERNEL;
        return p;
    }
    if (tokens > HADAMARD_MAX_NP) { p.path = HADAMARD_REFUSE_TOKENS; return p; }
    p.np = hadamard_next_pow2(tokens);
    if (!has_workspace) { p.path = HADAMARD_REFUSE_WORKSPACE; return p; }
    p.rpw = p.dp >= 512 ? 1 : 512 / p.dp;
    p.cs = (int)(HADAMARD_SLAB_LDS / 4 / (size_t)p.np);
    if (p.cs > 64) p.cs = 64;
    if (p.cs > p.dp) p.cs = p.dp;
    const size_t l1 = (size_t)p.rpw * p.dp * 4, l2 = (size_t)p.np * p.cs * 4;
    p.lds = l1 > l2 ? l1 : l2;
    p.path = HADAMARD_GENERIC;
    return p;
}

// fp32 workspace of the generic path: the row pass's output, cropped to dim columns.  A function of the shape only.
inline int64_t hadamard_workspace_floats(int batch, int tokens, int dim) {
    if (batch < 1) return 0;
    return hadamard_select(0, tokens, dim, true).path == HADAMARD_GENERIC ? (int64_t)batch * tokens * dim : 0;
}

inline int hadamard_ln_supported(int tokens, int dim, int dtype) {
    return (dtype == 1 && dim == HADAMARD_LN_DIM && tokens >= HADAMARD_LN_MIN_TOKENS && tokens <= HADAMARD_LN_MAX_TOKENS) ? 1 : 0;
}
inline int hadamard_cls_supported(int tokens, int dim, int dtype) {
    return ((dtype == 0 || dtype == 1) && (dim == 256 || dim == 512 || dim == 1024) && tokens >= 1) ? 1 : 0;
}
