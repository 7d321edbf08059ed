// The host side of spv_permut.hip's dispatch: the table geometry (which tables spv_permut_pack writes and where) and four pure
// selectors that name, for one call of an entry point, either the refusal or the ONE kernel that serves it.  The entry points switch
// on the selector's answer and do nothing else to choose.  No HIP type in it: tests/test_permut_ref.py compiles it with a plain C++
// compiler and holds every selector to the Python restatement tests/permut_edge_cases.py over a grid that straddles each threshold.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int PERMUT_PT = 1024;                 // threads per workgroup of the LDS kernels
constexpr int PERMUT_LDS_LIMIT = 150 * 1024;    // bytes of LDS a gather kernel asks for at most
constexpr int PERMUT_C_IT = 5;                  // compact backward: d <= 8 * PT * C_IT = 40 960
constexpr int PERMUT_MAX_IT = 10;               // wide backward:    d <= 4 * PT * MAX_IT = 40 960
constexpr int PERMUT_DT_F32 = 0, PERMUT_DT_BF16 = 1;   // SPV_F32, SPV_BF16

// compact tables exist iff every index fits 16 bits and head slices start on a sign-byte boundary
inline bool compact_ok(int d) { return d <= 65536 && d % 8 == 0; }
// a bf16 row that does not fit the LDS: spv_permut_pack appends the scatter lists
inline bool long_row(int d) { return (size_t)d * 2 > (size_t)PERMUT_LDS_LIMIT; }
inline int scat_parts(int d) { return (int)(((size_t)d * 4 + PERMUT_LDS_LIMIT - 1) / PERMUT_LDS_LIMIT); }
inline int scat_len(int d) { const int n = scat_parts(d); return (((d + n - 1) / n) + 7) / 8 * 8; }
inline int64_t scat_set_words(int heads, int d) {   // one list set: off, cur, ej, et
    const int64_t total = (int64_t)heads * d;
    return (int64_t)heads * (scat_parts(d) + 1) + (int64_t)heads * scat_parts(d) + total + (total + 1) / 2;
}
inline int64_t scat_words(int heads, int d) { return 2 * scat_set_words(heads, d); }   // [0] the backward's (from the forward table), [1] the forward's
inline int64_t permut_table_words(int heads, int d) {
    const int64_t total = (int64_t)heads * d;
    return 2 * total + (compact_ok(d) ? total + (total / 4 + 3) / 4 : 0) + (long_row(d) ? scat_words(heads, d) : 0);
}
// 1 when the scatter forward can emit `pooled` for this window: a shape-only answer (spv_permut_gather_fwd refuses a call whose x or
// g is not 16-byte aligned or whose batch exceeds 65 535 rather than leave `pooled` unwritten)
inline int permut_pool_supported(int heads, int d, int pool_window, int dtype) {
    return (dtype == PERMUT_DT_BF16 && long_row(d) && d % 8 == 0 && heads <= 65535 && pool_window > 0 && d % pool_window == 0 &&
            scat_len(d) % pool_window == 0) ? 1 : 0;
}

enum PermutPath : int {
    // refusals
    PERMUT_REFUSE_EMPTY = 0,         // a size is <= 0
    PERMUT_REFUSE_DTYPE,             // neither SPV_F32 nor SPV_BF16
    PERMUT_REFUSE_POOL_LDS,          // pooled: the row fits neither the LDS path nor the scatter path's windows
    PERMUT_REFUSE_POOL_WINDOW,       // pooled on the LDS path: window not 4 / 8 / 16 / 32, or a wave would straddle the table's end
    PERMUT_REFUSE_POOL_UNSERVED,     // pooled, and the call would fall through to a kernel that does not emit it
    PERMUT_REFUSE_ROW0_SHAPE,        // spv_permut_row0_*: n or embed outside (0, d], or (backward) d / embed not multiples of 8
    // forward
    PERMUT_FWD_PAIR,                 // gather_fwd_pair_kernel
    PERMUT_FWD_LDS,                  // gather_fwd_lds_kernel<T>
    PERMUT_FWD_SCATTER,              // gather_fwd_scatter_kernel
    PERMUT_FWD_GLOBAL,               // gather_fwd_global_kernel<T>
    // backward
    PERMUT_BWD_DMA,                  // gather_bwd_dma_kernel
    PERMUT_BWD_C16,                  // gather_bwd_c16_kernel
    PERMUT_BWD_LDS,                  // gather_bwd_lds_kernel<float>
    PERMUT_BWD_SCATTER,              // gather_bwd_scatter_kernel
    PERMUT_BWD_PARTS,                // gather_bwd_parts_kernel
    PERMUT_BWD_GLOBAL,               // gather_bwd_global_kernel<T>
    // token row 0
    PERMUT_ROW0_FWD_LDS,             // permut_row0_fwd_lds_kernel<T>
    PERMUT_ROW0_FWD_GLOBAL,          // permut_row0_fwd_kernel<T>
    PERMUT_ROW0_BWD_LDS,             // permut_row0_bwd_lds_kernel<T>
    PERMUT_ROW0_BWD_GLOBAL,          // permut_row0_init_kernel<T> + permut_row0_scatter_kernel<T>
    PERMUT_PATH_COUNT
};
inline const char* permut_path_name(int p) {
    static const char* const names[PERMUT_PATH_COUNT] = {
        "refuse_empty", "refuse_dtype", "refuse_pool_lds", "refuse_pool_window", "refuse_pool_unserved", "refuse_row0_shape",
        "fwd_pair", "fwd_lds", "fwd_scatter", "fwd_global",
        "bwd_dma", "bwd_c16", "bwd_lds", "bwd_scatter", "bwd_parts", "bwd_global",
        "row0_fwd_lds", "row0_fwd_global", "row0_bwd_lds", "row0_bwd_global"};
    return p >= 0 && p < PERMUT_PATH_COUNT ? names[p] : "?";
}

// x16 / g16 / idx16 (and dg16 / dx16 / x016 / dx016 below): that pointer is 16-byte aligned.  Every kernel but the global ones moves
// 16-, 8- or 4-byte pieces through these pointers; a call with one of them off alignment is served by the global kernel, whose
// accesses are one element wide -- or refused, when it asked for `pooled`, which the global kernel does not emit.
inline PermutPath permut_fwd_path(int dtype, int heads, int d, int batch, bool pooled, int pw, bool x16, bool g16, bool idx16) {
    if (batch <= 0 || heads <= 0 || d <= 0) return PERMUT_REFUSE_EMPTY;
    if (dtype != PERMUT_DT_F32 && dtype != PERMUT_DT_BF16) return PERMUT_REFUSE_DTYPE;
    const bool bf = dtype == PERMUT_DT_BF16;
    const size_t es = bf ? 2 : 4;
    const int64_t total = (int64_t)heads * d;
    const bool aligned = ((size_t)d * es) % 16 == 0 && total % 4 == 0;
    const bool fits = (size_t)d * es <= (size_t)PERMUT_LDS_LIMIT;
    // the scatter path emits any window that divides its quarters
    const bool scat_pool = pooled && bf && long_row(d) && pw > 0 && d % pw == 0 && scat_len(d) % pw == 0;
    if (pooled && !scat_pool) {
        if (!(aligned && fits)) return PERMUT_REFUSE_POOL_LDS;
        if (!((pw == 4 || pw == 8 || pw == 16 || pw == 32) && total % pw == 0 && (total / 4) % PERMUT_PT == 0)) return PERMUT_REFUSE_POOL_WINDOW;
    }
    const bool ptrs = x16 && g16 && idx16;
    PermutPath p;
    if (ptrs && bf && compact_ok(d) && (size_t)d * 4 <= (size_t)PERMUT_LDS_LIMIT &&
        (!pooled || ((pw == 8 || pw == 16 || pw == 32) && (total / 8) % PERMUT_PT == 0)))
        p = PERMUT_FWD_PAIR;
    else if (ptrs && aligned && fits)
        p = PERMUT_FWD_LDS;
    else if (bf && long_row(d) && d % 8 == 0 && x16 && g16 && heads <= 65535 && batch <= 65535)   // grid = (parts, heads, batch)
        p = PERMUT_FWD_SCATTER;
    else
        p = PERMUT_FWD_GLOBAL;
    return pooled && p == PERMUT_FWD_GLOBAL ? PERMUT_REFUSE_POOL_UNSERVED : p;
}

inline PermutPath permut_bwd_path(int dtype, int heads, int d, int batch, bool dg16, bool dx16, bool idx16) {
    if (batch <= 0 || heads <= 0 || d <= 0) return PERMUT_REFUSE_EMPTY;
    if (dtype != PERMUT_DT_F32 && dtype != PERMUT_DT_BF16) return PERMUT_REFUSE_DTYPE;
    const bool bf = dtype == PERMUT_DT_BF16;
    const size_t es = bf ? 2 : 4;
    const bool aligned = ((size_t)d * es) % 16 == 0 && d % 4 == 0;   // then the inverse table, heads * d words in, is aligned with idx
    const bool ptrs = dg16 && dx16 && idx16;
    if (ptrs && bf && compact_ok(d) && ((size_t)d * 2) % 1024 == 0 && (size_t)d * 4 <= (size_t)PERMUT_LDS_LIMIT && d <= 8 * PERMUT_PT * PERMUT_C_IT)
        return PERMUT_BWD_DMA;
    if (ptrs && bf && compact_ok(d) && (size_t)d * 2 <= (size_t)PERMUT_LDS_LIMIT && d <= 8 * PERMUT_PT * PERMUT_C_IT) return PERMUT_BWD_C16;
    if (ptrs && !bf && aligned && (size_t)d * es <= (size_t)PERMUT_LDS_LIMIT && d <= 4 * PERMUT_PT * PERMUT_MAX_IT) return PERMUT_BWD_LDS;
    // the scatter reads dg one element at a time and stores dx in 4-byte pieces
    if (bf && long_row(d) && d % 8 == 0 && dx16 && (size_t)scat_len(d) * 4 <= (size_t)PERMUT_LDS_LIMIT) return PERMUT_BWD_SCATTER;
    // one part: the whole gradient row of a head in LDS (40 960 < d <= 76 800)
    if (ptrs && bf && d % 8 == 0 && !long_row(d)) return PERMUT_BWD_PARTS;
    return PERMUT_BWD_GLOBAL;
}

inline PermutPath permut_row0_fwd_path(int dtype, int batch, int d, int n, int embed, bool x16, bool x016) {
    if (!(batch > 0 && d > 0 && n > 0 && n <= d && embed > 0 && embed <= d)) return PERMUT_REFUSE_ROW0_SHAPE;
    if (dtype != PERMUT_DT_F32 && dtype != PERMUT_DT_BF16) return PERMUT_REFUSE_DTYPE;
    const bool bf = dtype == PERMUT_DT_BF16;
    const size_t row_bytes = (size_t)d * (bf ? 2 : 4);
    const int vec = bf ? 8 : 4;
    return row_bytes <= (size_t)PERMUT_LDS_LIMIT && d % vec == 0 && embed % vec == 0 && x16 && x016 ? PERMUT_ROW0_FWD_LDS : PERMUT_ROW0_FWD_GLOBAL;
}

inline PermutPath permut_row0_bwd_path(int dtype, int batch, int d, int n, int embed, bool dx16, bool dx016) {
    if (!(batch > 0 && d > 0 && n > 0 && n <= d && embed > 0 && embed <= d && d % 8 == 0 && embed % 8 == 0)) return PERMUT_REFUSE_ROW0_SHAPE;
    if (dtype != PERMUT_DT_F32 && dtype != PERMUT_DT_BF16) return PERMUT_REFUSE_DTYPE;
    const size_t row_bytes = (size_t)d * (dtype == PERMUT_DT_BF16 ? 2 : 4);
    return row_bytes <= (size_t)PERMUT_LDS_LIMIT && dx16 && dx016 ? PERMUT_ROW0_BWD_LDS : PERMUT_ROW0_BWD_GLOBAL;
}
