// The split plan of a TN contraction launch (gemm_tn.hip): how the token range is cut over workgroups, what the workspace holds and the
// grids of the reductions -- pure functions of the shape, the K-tile length and VIPANT_TN_SPLIT.  Host-only header (nothing from HIP):
// tests/test_tn_plan_cpu.py compiles it alone (tests/tn_plan_main.cpp) and checks every field against tests/tn_plan.py.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

constexpr int64_t TN_TILE = 256;             // the output tile of a workgroup, TN_TILE x TN_TILE
constexpr int TN_BK = 64, TN_BK8 = 128;      // tokens per K-tile: bf16 kernels, e4m3 kernel

struct TnPlan {
    int64_t ntp, ntq, tiles;      // output tiles of ONE problem
    int nk, splits, per;          // K-tiles of the token range; workgroups per tile and K-tiles of each (the last may be shorter)
    bool direct;                  // one split and nothing to accumulate: the kernel stores into C, no reduction
    // the workspace: the fp32 partial tiles [problem][split][tile] first, then the column-sum partials [split * ntq][ntp * 256]
    size_t slab_bytes;            // per problem
    size_t colsum_bytes;          // 0 for a pair
    size_t workspace_bytes;
    int reduce_blocks;            // per problem, 256 threads x 4 floats each, grid-stride beyond the cap
    int cs_parts, cs_stride;      // partial vectors per column sum, floats between two of them
};

// VIPANT_TN_SPLIT=k (experiment, default 1): k times as many, k times shorter workgroups per weight-gradient launch -- several per CU
// instead of one long one, so that CUs another stream's kernel holds (the replica group's all-reduce) cost a launch 1/k of a workgroup's
// time at its tail instead of a whole one; the price is k times the partial tiles to write and reduce (profiles/r6_comm_shadow_cfg5.md).
// The entry points read the variable on every call.
static inline int tn_split_factor(const char* env_value) {
    const int k = env_value ? atoi(env_value) : 1;
    return k < 1 ? 1 : (k > 8 ? 8 : k);
}

// `problems`: 1, or 2 for vipant_gemm_tn_pair -- both problems' tiles share the chip, the factor does not apply, nothing accumulates and
// there are no column sums
static inline TnPlan tn_plan(int64_t M, int64_t P, int64_t Q, int bk, int problems, int factor, bool accumulate) {
    const auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    const bool pair = problems == 2;
    if (pair) { factor = 1; accumulate = false; }
    TnPlan pl;
    pl.ntp = ceil_div(P, TN_TILE);
    pl.ntq = ceil_div(Q, TN_TILE);
    pl.tiles = pl.ntp * pl.ntq;
    const int64_t in_plan = problems * pl.tiles, nk = ceil_div(M, bk);
    int64_t s = 256 / in_plan * (in_plan <= 256 ? factor : 1);      // fill 256 CUs
    if (s < 1) s = 1;
    if (s > nk) s = nk;
    const int64_t per = ceil_div(nk, s);
    pl.nk = (int)nk;
    pl.per = (int)per;
    pl.splits = (int)ceil_div(nk, per);
    pl.direct = pl.splits == 1 && !accumulate;
    pl.slab_bytes = (size_t)pl.splits * (size_t)pl.tiles * TN_TILE * TN_TILE * sizeof(float);
    pl.cs_parts = (int)(pl.splits * pl.ntq);
    pl.cs_stride = (int)(pl.ntp * TN_TILE);
    pl.colsum_bytes = pair ? 0 : (size_t)pl.cs_parts * (size_t)pl.cs_stride * sizeof(float);
    pl.workspace_bytes = problems * pl.slab_bytes + pl.colsum_bytes;
    const int64_t blocks = ceil_div(pl.tiles * TN_TILE * TN_TILE / 4, 256), cap = pair ? 1024 : 2048;
    pl.reduce_blocks = (int)(blocks > cap ? cap : blocks);
    return pl;
}
