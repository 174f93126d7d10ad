// LayerNorm forward / backward at the widths D = 64 H that are no multiple of 256: H = 3, 5, 6, 7, 9, 10, 11, 13, 14, 15 (192 .. 960).
// Same arguments, semantics and `partial` layout as ln_fwd_kernel / ln_bwd_kernel (layernorm.hip), which keep the multiples of 256;
// vipant_layernorm_fwd / _bwd dispatch here (ln_widths_fwd / ln_widths_bwd below).  No e4m3 output at these widths.
//
// The split.  A row is CH = 16 H chunks of four elements (16 bytes of fp32, 8 of fp16 / bf16), which 64 lanes do not divide when
// H % 4 != 0.  A row therefore belongs to a GROUP of L = 16, 32 or 64 lanes (64 / L rows per wave); lane gl of the group owns the
// chunks t L + gl, t = 0 .. C - 1, C = ceil(CH / L).  When L does not divide CH the last step is ragged: only the lanes with
// (C - 1) L + gl < CH own a chunk there, the others carry zeros through the reductions and touch no memory.  L = 16 divides every CH
// (no ragged step, 4 rows per wave), L = 32 every even H; L = 64 is one wave per row with a ragged last step.  The reductions stay
// inside the group: four DPP steps inside a row of 16 lanes, then one / two cross-row exchanges for L = 32 / 64.
#include <type_traits>

#include "common.h"

namespace {

constexpr float LN_EPS = 1e-5f;

typedef _Float16 f16_t;
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 load_stream4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 load_stream4(const f16_t* p) {
    const f16x4 h = *(const f16x4*)p;
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
__device__ __forceinline__ void store_stream4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void store_stream4(f16_t* p, f32x4 v) {
    f16x4 h;
    h[0] = (f16_t)v[0]; h[1] = (f16_t)v[1]; h[2] = (f16_t)v[2]; h[3] = (f16_t)v[3];
    *(f16x4*)p = h;
}

// Lanes per row, by H.  Groups of 16 / 32 lanes keep every lane busy and 4 / 2 rows per wave in flight where a row is short; from
// H = 9 a lane of a 64-lane group already holds three or four chunks (what the D = 768 / 1024 kernels of layernorm.hip hold), and
// narrower groups would only add registers: the backward keeps gamma, three column accumulators and two rows in flight per chunk
// (~45 registers per chunk with fp32 operands): at H = 5 a 16-lane group (C = 5) compiles to 256 VGPRs + up to 58 AGPRs, so groups
// of 16 stop at C = 3 and 320 takes 32 lanes with a ragged third step.  Measured: profiles/ln_widths_observed.txt.
// VIPANT_LN_LANES (a compile-time definition, timing builds only) forces one group size for every width.
constexpr int ln_lanes(int H) {
#ifdef VIPANT_LN_LANES
    return VIPANT_LN_LANES;
#else
    return H <= 3 ? 16 : (H <= 7 ? 32 : 64);
#endif
}

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// Sum over the aligned group of L lanes, the same bits in every lane of it.  Only lanes of the group are read, so groups of one
// wave may sit in different iterations of their row loops (a group is either all in or all out).
template <int L>
__device__ __forceinline__ float group_sum(float v) {
    v = dpp_add<0xB1>(v);       // quad_perm [1, 0, 3, 2]
    v = dpp_add<0x4E>(v);       // quad_perm [2, 3, 0, 1]
    v = dpp_add<0x141>(v);      // row_half_mirror: the other quad of the eight
    v = dpp_add<0x140>(v);      // row_mirror: the other eight of the sixteen
    if (L >= 32) v += __shfl_xor(v, 16, 64);
    if (L == 64) v += __shfl_xor(v, 32, 64);
    return v;
}

template <int H, int L>
struct Split {
    static_assert(L == 16 || L == 32 || L == 64, "a group is 16, 32 or 64 lanes");
    static constexpr int D = 64 * H, CH = 16 * H, C = (CH + L - 1) / L, RPW = 64 / L;
    static constexpr bool RAGGED = CH % L != 0;
};

template <int H, int L, typename XI, typename XO>  // XI / XO: the stream's element type on the way in / out
__global__ __launch_bounds__(256) void lnw_fwd_kernel(const XI* __restrict__ x, int64_t ldx, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                      float* __restrict__ y32, float* __restrict__ mean,
                                                      float* __restrict__ rstd, int64_t M, const bf16_t* __restrict__ add,
                                                      XO* __restrict__ sum_out) {
    using S = Split<H, L>;
    constexpr int D = S::D, C = S::C;
    const int lane = threadIdx.x & 63, gl = lane & (L - 1);
    const int64_t grp = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * S::RPW + lane / L;
    const int64_t ngrp = (int64_t)gridDim.x * 4 * S::RPW;
    const bool tail = !S::RAGGED || (C - 1) * L + gl < S::CH;      // this lane owns a chunk in the last step
    auto live = [&](int t) { return t < C - 1 || tail; };
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 gv[C], bv[C];
#pragma unroll
    for (int t = 0; t < C; ++t) {
        gv[t] = live(t) ? *(const f32x4*)(gamma + (t * L + gl) * 4) : zero;
        bv[t] = live(t) ? *(const f32x4*)(beta + (t * L + gl) * 4) : zero;
    }
    for (int64_t row = grp; row < M; row += ngrp) {
        const XI* xr = x + row * ldx;
        f32x4 v[C];
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < C; ++t) {
            v[t] = zero;
            if (live(t)) {
                const int col = (t * L + gl) * 4;
                v[t] = load_stream4(xr + col);
                if (add != nullptr) {      // residual add fused in front of the norm: v = x + branch (bf16)
                    const bf16x4 a4 = *(const bf16x4*)(add + row * D + col);
                    v[t] += f32x4{(float)a4[0], (float)a4[1], (float)a4[2], (float)a4[3]};
                    // the new stream is stored in its own precision; the norm below works on the unrounded sum
                    if (sum_out != nullptr) store_stream4(sum_out + row * D + col, v[t]);
                }
            }
            s += v[t][0] + v[t][1] + v[t][2] + v[t][3];
        }
        const float mu = group_sum<L>(s) * (1.0f / D);
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < C; ++t) {
            v[t] = live(t) ? v[t] - mu : zero;
            q += v[t][0] * v[t][0] + v[t][1] * v[t][1] + v[t][2] * v[t][2] + v[t][3] * v[t][3];
        }
        const float rs = rsqrtf(group_sum<L>(q) * (1.0f / D) + LN_EPS);
#pragma unroll
        for (int t = 0; t < C; ++t) {
            if (!live(t)) continue;
            const f32x4 o = v[t] * rs * gv[t] + bv[t];
            const int64_t off = row * D + (t * L + gl) * 4;
            if (y != nullptr) *(bf16x4*)(y + off) = f32x4_to_bf16x4(o);
            if (y32 != nullptr) *(f32x4*)(y32 + off) = o;
        }
        if (gl == 0) { mean[row] = mu; rstd[row] = rs; }
    }
}

// dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma,  xhat = (x - mean) * rstd; per-block partial sums of
// dgamma, dbeta and the column sums of dx go to `partial` [grid, 3, D] (ln_bwd_finalize_kernel folds them).  Persistent: group g
// of the grid takes rows g, g + ngrp, ..., two of them in flight (the ring of ln_bwd_kernel, per group instead of per wave).
template <int H, int L, bool DY_F32, bool DRES_BF16, typename XT>
__global__ __launch_bounds__(256) void lnw_bwd_kernel(const void* __restrict__ dy_, const XT* __restrict__ x, int64_t ldx,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma, const void* dres_, float* dx, int64_t lddx,
                                                      bf16_t* dxb, float* __restrict__ partial, int64_t M) {
    using S = Split<H, L>;
    constexpr int D = S::D, C = S::C, NWV = 4, G = NWV * S::RPW;      // G groups (rows in one round) per workgroup
    static_assert(G * D * sizeof(float) <= 64 * 1024, "the column-sum reduction buffer must fit the LDS");
    const float* dres = DRES_BF16 ? nullptr : (const float*)dres_;
    const bf16_t* dresb = DRES_BF16 ? (const bf16_t*)dres_ : nullptr;
    const int lane = threadIdx.x & 63, gl = lane & (L - 1);
    const int gidx = (threadIdx.x >> 6) * S::RPW + lane / L;          // the group within the workgroup
    const int64_t grp = (int64_t)blockIdx.x * G + gidx;
    const int64_t ngrp = (int64_t)gridDim.x * G;
    const bool tail = !S::RAGGED || (C - 1) * L + gl < S::CH;
    auto live = [&](int t) { return t < C - 1 || tail; };
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 gv[C], dg[C], db[C], dsum[C];
#pragma unroll
    for (int t = 0; t < C; ++t) {
        gv[t] = live(t) ? *(const f32x4*)(gamma + (t * L + gl) * 4) : zero;
        dg[t] = zero; db[t] = zero; dsum[t] = zero;
    }
    using DyT = typename std::conditional<DY_F32, float, bf16_t>::type;
    using DyRaw = typename std::conditional<DY_F32, f32x4, bf16x4>::type;
    using XRaw = typename std::conditional<sizeof(XT) == 4, f32x4, f16x4>::type;
    struct Raw { DyRaw dy[C]; XRaw x[C]; bf16x4 rb[C]; f32x4 rf[C]; float mu, rs; };
    auto load_row = [&](int64_t row, Raw& r) {
        r.mu = mean[row]; r.rs = rstd[row];
#pragma unroll
        for (int t = 0; t < C; ++t) {
            if (!live(t)) continue;
            const int col = (t * L + gl) * 4;
            r.dy[t] = *(const DyRaw*)((const DyT*)dy_ + row * D + col);
            r.x[t] = *(const XRaw*)(x + row * ldx + col);
            if (DRES_BF16) r.rb[t] = *(const bf16x4*)(dresb + row * D + col);
            else if (dres != nullptr) r.rf[t] = *(const f32x4*)(dres + row * lddx + col);
        }
    };
    auto reduce_row = [&](int64_t row, const Raw& r) {
        const float mu = r.mu, rs = r.rs;
        f32x4 xh[C], g[C];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int t = 0; t < C; ++t) {
            xh[t] = zero; g[t] = zero;
            if (!live(t)) continue;             // (an idle lane of the ragged step adds zeros to the row's two sums)
            f32x4 dyv, xv;
#pragma unroll
            for (int e = 0; e < 4; ++e) { dyv[e] = (float)r.dy[t][e]; xv[e] = (float)r.x[t][e]; }
            xh[t] = (xv - mu) * rs;
            g[t] = dyv * gv[t];
            dg[t] += dyv * xh[t];
            db[t] += dyv;
            s1 += g[t][0] + g[t][1] + g[t][2] + g[t][3];
            s2 += g[t][0] * xh[t][0] + g[t][1] * xh[t][1] + g[t][2] * xh[t][2] + g[t][3] * xh[t][3];
        }
        s1 = group_sum<L>(s1) * (1.0f / D);
        s2 = group_sum<L>(s2) * (1.0f / D);
#pragma unroll
        for (int t = 0; t < C; ++t) {
            if (!live(t)) continue;
            const int col = (t * L + gl) * 4;
            f32x4 o = (g[t] - s1 - xh[t] * s2) * rs;
            if (DRES_BF16) o += f32x4{(float)r.rb[t][0], (float)r.rb[t][1], (float)r.rb[t][2], (float)r.rb[t][3]};
            else if (dres != nullptr) o += r.rf[t];
            dsum[t] += o;
            if (dx != nullptr) *(f32x4*)(dx + row * lddx + col) = o;
            if (dxb != nullptr) *(bf16x4*)(dxb + row * D + col) = f32x4_to_bf16x4(o);
        }
    };
    Raw ring[2];
    if (grp < M) load_row(grp, ring[0]);
    for (int64_t row = grp; row < M; row += 2 * ngrp) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t r = row + i * ngrp;
            if (r + ngrp < M) load_row(r + ngrp, ring[i ^ 1]);
            if (r < M) reduce_row(r, ring[i]);
        }
    }
    // the workgroup's G groups fold their column sums through a [G][D] LDS buffer, one quantity at a time; an idle lane of the
    // ragged step owns no column and writes nothing, the sweep below reads columns 0 .. D - 1 only
    __shared__ float red[G * D];
#pragma unroll
    for (int which = 0; which < 3; ++which) {
#pragma unroll
        for (int t = 0; t < C; ++t)
            if (live(t)) *(f32x4*)(red + gidx * D + (t * L + gl) * 4) = which == 0 ? dg[t] : (which == 1 ? db[t] : dsum[t]);
        __syncthreads();
        for (int i = threadIdx.x; i < D; i += NWV * 64) {
            float acc = 0.f;
#pragma unroll
            for (int w = 0; w < G; ++w) acc += red[w * D + i];
            partial[((int64_t)blockIdx.x * 3 + which) * D + i] = acc;
        }
        __syncthreads();
    }
}

}  // namespace

#define LN_WIDTHS(X) X(3) X(5) X(6) X(7) X(9) X(10) X(11) X(13) X(14) X(15)

int32_t ln_widths_fwd(const void* x, int64_t ldx, const float* gamma, const float* beta, bf16_t* y, float* y32, float* mean,
                      float* rstd, int64_t M, int64_t D, const bf16_t* add, void* sum_out, bool in16, bool out16, hipStream_t s) {
#define LNW_FWD_T(H, XI, XO)                                                                                                      \
    hipLaunchKernelGGL((lnw_fwd_kernel<H, ln_lanes(H), XI, XO>), dim3(blocks), dim3(256), 0, s, (const XI*)x, ldx, gamma, beta, y, \
                       y32, mean, rstd, M, add, (XO*)sum_out)
#define LNW_FWD(H)                                                                                       \
    case H: {                                                                                            \
        const int64_t nb = ceil_div(M, 4 * (64 / ln_lanes(H)));      /* one row per group, as one row per wave in ln_fwd_kernel */ \
        const int blocks = (int)(nb > (1 << 20) ? (1 << 20) : nb);                                       \
        if (in16 && out16) LNW_FWD_T(H, f16_t, f16_t);                                                   \
        else if (in16) LNW_FWD_T(H, f16_t, float);                                                       \
        else if (out16) LNW_FWD_T(H, float, f16_t);                                                      \
        else LNW_FWD_T(H, float, float);                                                                 \
    } break;
    switch (D / 64) {
        LN_WIDTHS(LNW_FWD)
        default: VIPANT_REQUIRE(false, VIPANT_EBADSHAPE, "layernorm_fwd: no kernel for D=%ld", (long)D);
    }
#undef LNW_FWD
#undef LNW_FWD_T
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

int32_t ln_widths_bwd(const void* dy, bool dy_is_f32, bool dres_bf16, bool x16, const void* x, int64_t ldx, const float* mean,
                      const float* rstd, const float* gamma, const void* dres, float* dx, int64_t lddx, bf16_t* dxb, float* partial,
                      int blocks, int64_t M, int64_t D, hipStream_t s) {
#define LNW_BWD_T(H, A, B, XT)                                                                                                    \
    hipLaunchKernelGGL((lnw_bwd_kernel<H, ln_lanes(H), A, B, XT>), dim3(blocks), dim3(256), 0, s, dy, (const XT*)x, ldx, mean, rstd, \
                       gamma, dres, dx, lddx, dxb, partial, M)
#define LNW_BWD(H)                                                                                                      \
    case H:                                                                                                             \
        if (dy_is_f32) { if (x16) LNW_BWD_T(H, true, false, f16_t); else LNW_BWD_T(H, true, false, float); }            \
        else if (dres_bf16) { if (x16) LNW_BWD_T(H, false, true, f16_t); else LNW_BWD_T(H, false, true, float); }       \
        else { if (x16) LNW_BWD_T(H, false, false, f16_t); else LNW_BWD_T(H, false, false, float); }                    \
        break;
    switch (D / 64) {
        LN_WIDTHS(LNW_BWD)
        default: VIPANT_REQUIRE(false, VIPANT_EBADSHAPE, "layernorm_bwd: no kernel for D=%ld", (long)D);
    }
#undef LNW_BWD
#undef LNW_BWD_T
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}
