// The host side of the token-embedding forward kernel (spv_patch.hip: token_embed_kernel): which calls it serves and how its grid is
// sized.  spv_token_embed_supported / spv_token_embed_fwd answer from these two functions and do nothing else to choose.  No HIP type
// in it: tests/test_token_embed_host.py holds the selector to a Python restatement over a grid that straddles each limit.
#pragma once
#include <stdint.h>

constexpr int TE_ROWS = 32, TE_COLS = 64;   // one wave's output block: a 32-row block of the tokens x one 128-byte line of each row
constexpr int TE_WAVES = 4;                 // waves per workgroup (independent of one another: no workgroup barrier in the kernel)
constexpr int TE_WAVES_PER_CU = 12;         // resident waves per CU the grid is sized for (3 per SIMD: the kernel holds 141 VGPRs at K = 48, 153 at K = 64)
constexpr int TE_DT_BF16 = 1;               // SPV_BF16

// bf16 in and out; K of 1..4 MFMA steps of 16 (3 x 4 x 4 = 48: CIFAR, 1 x 4 x 4 = 16: MNIST); whole 64-column shares
inline int token_embed_supported(int rows, int n, int k, int dtype) {
    return dtype == TE_DT_BF16 && rows > 0 && n > 0 && n % TE_COLS == 0 && k >= 16 && k <= 64 && k % 16 == 0;
}

// A wave keeps ONE 64-column share of the weight in registers for its whole life and walks 32-row blocks: `walkers` waves per share,
// wave g of the grid serving share g % shares as walker g / shares over blocks walker, walker + walkers, ...  The walkers are as many as
// the resident-wave budget allows, then cut back to the fewest that keep the longest walk (`per` blocks) as it is, so the shares are
// even up to one block.
struct TokenEmbedPlan {
    int shares, walkers, per, grid;
};
inline TokenEmbedPlan token_embed_plan(int rows, int n, int cus) {
    TokenEmbedPlan p{};
    p.shares = n / TE_COLS;
    const int nblk = (int)(((int64_t)rows + TE_ROWS - 1) / TE_ROWS);
    int most = (int)((int64_t)cus * TE_WAVES_PER_CU / p.shares);
    if (most < 1) most = 1;
    p.per = (nblk + most - 1) / most;
    p.walkers = (nblk + p.per - 1) / p.per;
    p.grid = (int)(((int64_t)p.walkers * p.shares + TE_WAVES - 1) / TE_WAVES);
    return p;
}
