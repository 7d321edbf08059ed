// The host side of spv_gfilter.hip (the learnable global-filter token mixer): one pure selector that names, for a shape, either the
// refusal or the kernel plan that serves it, and the sizes of the table, the workspace and the filter-gradient slabs.  The entry points
// switch on these answers and do nothing else to choose; spv_gfilter_path returns the selector's code.  No HIP type in it: it compiles
// with a plain C++ compiler, and tests/gfilter_ref.py restates it in Python.
#pragma once
#include <stddef.h>
#include <stdint.h>

// codes of spv_gfilter_path (include/spv.h names the same values)
constexpr int GFILTER_FAST = 1;                // gfilter_fast_fwd_kernel / gfilter_fast_bwd_kernel: both token-axis products on the MFMA
constexpr int GFILTER_GENERIC = 2;             // gfilter_fwd_kernel<T> / gfilter_bwd_kernel<T> (+ gfilter_fold_kernel): fp32 in LDS
constexpr int GFILTER_REFUSE_EMPTY = -1;       // tokens < 1 or dim < 1
constexpr int GFILTER_REFUSE_DTYPE = -2;       // neither SPV_F32 (0) nor SPV_BF16 (1)
constexpr int GFILTER_REFUSE_TOKENS = -3;      // the table and one column of the backward (4 tokens + 4 bins floats) no longer fit the LDS budget

constexpr int GFILTER_REFUSE_ALIGN = -4;       // a shape of the fast window whose pointers are not 16-byte aligned

constexpr int GFILTER_FAST_MAX_TOKENS = 80;    // the fast window: bf16, dim % 64 == 0, tokens <= 80 (five K steps of 16, three row tiles of 32)
constexpr int GFILTER_FAST_COLS = 64;
constexpr int GFILTER_LDS_FLOATS = 16384;      // 64 KiB: what a workgroup gets without asking for more
constexpr int GFILTER_MAX_COLS = 64;           // columns of a workgroup = lanes of a wave
constexpr int GFILTER_MAX_SLABS = 32;          // sample groups of the backward = fp32 slabs of the filter gradient

constexpr int gfilter_bins(int tokens) { return tokens / 2 + 1; }

struct GfilterPlan {
    int path;            // one of the codes above
    int bins;            // K = tokens / 2 + 1 (0 when refused before it is formed)
    int cols_fwd;        // columns per workgroup of the forward: its LDS holds the table (2 tokens floats) and tokens + 2 K floats per column
    int cols_bwd;        // ... of the backward: 2 tokens + 4 K floats per column
};

inline int gfilter_cols(int tokens, int per_col, int dim) {
    int c = (GFILTER_LDS_FLOATS - 2 * tokens) / per_col;
    if (c > GFILTER_MAX_COLS) c = GFILTER_MAX_COLS;
    if (c > dim) c = dim;
    return c;
}

inline bool gfilter_fast_window(int dtype, int tokens, int dim) {
    return dtype == 1 && tokens >= 1 && tokens <= GFILTER_FAST_MAX_TOKENS && dim >= 1 && dim % GFILTER_FAST_COLS == 0;
}
// padded sizes of the fast path: the tokens as a K axis (steps of 16) and as output rows (tiles of 32), the bins as rows and K axis
constexpr int gfilter_fast_np(int tokens) { return (tokens + 15) / 16 * 16; }
constexpr int gfilter_fast_npo(int tokens) { return (tokens + 31) / 32 * 32; }
constexpr int gfilter_fast_kp(int tokens) { return gfilter_bins(tokens) <= 32 ? 32 : 64; }
// bf16 entries of the fast tables: T1 [hi, lo][cos, sin][KP][NP] (bins x tokens), then T2 [hi, lo][cos, sin][NPO][KP] (tokens x bins)
inline int64_t gfilter_fast_t1(int tokens) { return 4 * (int64_t)gfilter_fast_kp(tokens) * gfilter_fast_np(tokens); }
inline int64_t gfilter_fast_t2(int tokens) { return 4 * (int64_t)gfilter_fast_npo(tokens) * gfilter_fast_kp(tokens); }
// floats of the generic table, rounded up so that the fast tables behind it start on 16 bytes
inline int64_t gfilter_generic_table_floats(int tokens) { return (2 * (int64_t)tokens + 3) / 4 * 4; }

inline GfilterPlan gfilter_select(int dtype, int tokens, int dim, bool aligned) {
    GfilterPlan p = {GFILTER_REFUSE_EMPTY, 0, 0, 0};
    if (tokens < 1 || dim < 1) return p;
    if (dtype != 0 && dtype != 1) { p.path = GFILTER_REFUSE_DTYPE; return p; }
    if (tokens > (GFILTER_LDS_FLOATS - 4) / 6) { p.path = GFILTER_REFUSE_TOKENS; return p; }   // 2 N + 2 N + 4 (N / 2 + 1) <= 6 N + 4
    p.bins = gfilter_bins(tokens);
    if (gfilter_fast_window(dtype, tokens, dim)) {
        p.cols_fwd = p.cols_bwd = GFILTER_FAST_COLS;
        p.path = aligned ? GFILTER_FAST : GFILTER_REFUSE_ALIGN;
        return p;
    }
    p.cols_fwd = gfilter_cols(tokens, tokens + 2 * p.bins, dim);
    p.cols_bwd = gfilter_cols(tokens, 2 * tokens + 4 * p.bins, dim);
    p.path = GFILTER_GENERIC;
    return p;
}

// the DFT tables of one token count: (cos, sin)(2 pi j / tokens), j < tokens, fp32; inside the fast window's token range the bf16
// hi + lo matrices of the fast path follow, whatever dim and dtype the caller will use them with
inline int64_t gfilter_table_floats(int tokens) {
    if (tokens < 1) return 0;
    if (tokens > GFILTER_FAST_MAX_TOKENS) return 2 * (int64_t)tokens;
    return gfilter_generic_table_floats(tokens) + (gfilter_fast_t1(tokens) + gfilter_fast_t2(tokens)) / 2;
}

// fp32 workspace of a call: every kernel keeps the spectrum in LDS and needs none.  A function of the shape only.
inline int64_t gfilter_workspace_floats(int batch, int tokens, int dim) {
    (void)batch; (void)tokens; (void)dim;
    return 0;
}

// the backward's sample groups: workgroup (group g, column block) owns samples g, g + groups, ... and writes ONE slab
inline int gfilter_slabs(int batch) { return batch < 1 ? 0 : (batch < GFILTER_MAX_SLABS ? batch : GFILTER_MAX_SLABS); }

// fp32 slabs of the filter gradient: [slabs][K][dim][2], folded into dW in a fixed order
inline int64_t gfilter_partial_floats(int batch, int tokens, int dim) {
    if (batch < 1 || tokens < 1 || dim < 1) return 0;
    return (int64_t)gfilter_slabs(batch) * gfilter_bins(tokens) * dim * 2;
}
