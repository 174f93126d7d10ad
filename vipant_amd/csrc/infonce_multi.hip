// Several symmetric InfoNCE terms over shared feature matrices in one call (VACELossHead, cvap/module/decoder/loss_head.py:498-598):
//   loss = sum_k w_k (CE(s_k x_a x_b^T) + CE(s_k x_b x_a^T)),  k over up to five pairs (a_k, b_k) of up to five operands.
//
// Fused path (B <= 768, E = 512: the step's own batch), three launches whatever the pair count:
//   prep   every operand once: the hi / lo bf16 split [B][hi | lo] and the transposed bf16 copy [E][Bp32];
//   lse    workgroup (key chunk of 128, block of 16 queries, (pair, side)): infonce.hip's nce_rows_lse_kernel, the operands picked
//          by the pair table.  The three MFMA terms run in that kernel's order (x_a in the role of x1: [hi | hi | lo], x_b in the
//          role of x2: [hi | lo | hi]), so a pair's logits are the single-pair call's, bit for bit;
//   grad   workgroup (block of 16 rows, OPERAND, 128 columns): walks the operand's pairs in ascending k, and for each forms
//          s_k w_k dZ_k of its rows in registers as the MFMA operand against the transposed copy of the pair's other operand --
//          one set of accumulators for all pairs, i.e. the sum over pairs is a longer K loop: no adds, no atomics on dx.
// The first workgroup of every operand also sums its (pair, side) shares of the loss and of d logit_scale: two commutative terms
// per pair; the last of the 2 npair arrivals (a ticket) writes loss[0 .. npair] and dlogit_scale.
// The kernels restate nce_rows_* of infonce.hip with other operand addressing ([hi | lo] rows + K-segment offsets, per-pair strides,
// the loop over pairs) instead of sharing them through a policy-templated header; they run on the fused shapes only, where
// tests/test_infonce_multi_gpu.py pins them to the single-pair call bit for bit.
//
// Every other shape: the pairs one after another through vipant_infonce_fwd_bwd into workspace temporaries, added into dx in
// ascending k by a small vector kernel (same contract, same determinism).
#include "common.h"
#include <stdlib.h>

namespace {

constexpr int MAXN = 5;                             // operands, pairs
constexpr int ROWS_MAX_B = 768, ROWS_E = 512;       // the row-block shapes of infonce.hip

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct MultiWs {
    const float* x[MAXN];
    float* dx[MAXN];
    int pa[MAXN], pb[MAXN];
    float smax[MAXN], wt[MAXN];
    int nop, npair;
    bf16_t *xhl, *xt;                   // [nop][B][2 E] hi | lo;  [nop][E][Bp32]
    float *zws, *pmax, *psum, *pwz;     // [npair][2][B][Bp128];  [npair][2][KC][B] x 3
    float *diag, *scal, *accum;         // [npair][B];  [npair][2] (s, clamped);  [npair][2] sums + the ticket at [2 MAXN]
    int Bp32, Bp128, KC;
    size_t total;
};

MultiWs carve(char* base, int64_t B, int64_t E, int nop, int npair) {
    MultiWs w{};
    w.nop = nop; w.npair = npair;
    w.Bp32 = (int)((B + 31) / 32 * 32); w.Bp128 = (int)((B + 127) / 128 * 128); w.KC = w.Bp128 / 128;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += align256(bytes); return p; };
    w.xhl = (bf16_t*)take((size_t)nop * B * 2 * E * 2);
    w.xt = (bf16_t*)take((size_t)nop * E * w.Bp32 * 2);
    w.zws = (float*)take((size_t)npair * 2 * B * w.Bp128 * 4);
    w.pmax = (float*)take((size_t)npair * 2 * w.KC * B * 4);
    w.psum = (float*)take((size_t)npair * 2 * w.KC * B * 4);
    w.pwz = (float*)take((size_t)npair * 2 * w.KC * B * 4);
    w.diag = (float*)take((size_t)npair * B * 4);
    w.scal = (float*)take(256);
    w.accum = (float*)take(256);
    w.total = off;
    return w;
}

// a[i] of a table that lives in the kernel's arguments: selects over constant indices (a run-time index would move the table to scratch)
template <class T>
__device__ __forceinline__ T pick(const T (&a)[MAXN], int i) {
    T v = a[0];
#pragma unroll
    for (int k = 1; k < MAXN; ++k) v = i == k ? a[k] : v;
    return v;
}

__global__ __launch_bounds__(256) void ncem_prep_kernel(MultiWs w, const float* __restrict__ logit_scale, int B, int E) {
    const int op = blockIdx.y;
    if (blockIdx.x == 0 && op == 0) {
        if ((int)threadIdx.x < w.npair) {
            const float raw = __expf(logit_scale[threadIdx.x]);
            const float smax = pick(w.smax, (int)threadIdx.x);
            const bool clamped = smax > 0.f && raw > smax;
            w.scal[2 * threadIdx.x] = clamped ? smax : raw;
            w.scal[2 * threadIdx.x + 1] = clamped ? 1.f : 0.f;
        }
        if (threadIdx.x < 2 * MAXN + 1) w.accum[threadIdx.x] = 0.f;
    }
    const float* __restrict__ x = pick(w.x, op);
    bf16_t* xt = w.xt + (int64_t)op * E * w.Bp32;           // bf16(x)^T, columns B .. Bp32 zero
    const int64_t tt = (int64_t)E * w.Bp32;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tt; i += (int64_t)gridDim.x * 256) {
        const int n = (int)(i % w.Bp32);
        const int64_t e = i / w.Bp32;
        xt[i] = n < B ? (bf16_t)x[(int64_t)n * E + e] : (bf16_t)0.f;
    }
    bf16_t* xhl = w.xhl + (int64_t)op * B * 2 * E;
    const int64_t total = (int64_t)B * E;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / E;
        const int c = (int)(i % E);
        const float a = x[i];
        const bf16_t ah = (bf16_t)a;
        bf16_t* p = xhl + r * 2 * E + c;
        p[0] = ah; p[E] = (bf16_t)(a - (float)ah);
    }
}

template <int E>
__global__ __launch_bounds__(256) void ncem_lse_kernel(MultiWs w, int B) {
    __shared__ float red[4][3][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int kc = blockIdx.x, blk = blockIdx.y, pair = blockIdx.z >> 1, side = blockIdx.z & 1;
    constexpr int KS = 3 * E / 32, SEG = E / 32;
    const bf16_t* X1 = w.xhl + (int64_t)pick(w.pa, pair) * B * 2 * E;
    const bf16_t* X2 = w.xhl + (int64_t)pick(w.pb, pair) * B * 2 * E;
    const bf16_t* Q = side == 0 ? X1 : X2;
    const bf16_t* Kx = side == 0 ? X2 : X1;
    // the K segments of the two roles: x1 = [hi | hi | lo], x2 = [hi | lo | hi]
    const int qseg[3] = {0, side == 0 ? 0 : E, side == 0 ? E : 0};
    const int kseg[3] = {0, side == 0 ? E : 0, side == 0 ? 0 : E};
    const int m = 16 * blk + r;
    const bf16_t* qp = Q + (int64_t)(m < B ? m : B - 1) * 2 * E + 8 * g;
    const bf16_t* kp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = 128 * kc + 32 * wave + 16 * t + r;
        kp[t] = Kx + (int64_t)(n < B ? n : B - 1) * 2 * E + 8 * g;
    }
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    constexpr int HALF = KS / 2;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        bf16x8 qf[HALF];
#pragma unroll
        for (int s = 0; s < HALF; ++s) {
            const int st = half * HALF + s;
            qf[s] = *(const bf16x8*)(qp + qseg[st / SEG] + 32 * (st % SEG));
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            bf16x8 kf[HALF];
#pragma unroll
            for (int s = 0; s < HALF; ++s) {
                const int st = half * HALF + s;
                kf[s] = *(const bf16x8*)(kp[t] + kseg[st / SEG] + 32 * (st % SEG));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < HALF; ++s) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[s], qf[s], acc[t], 0, 0, 0);
        }
    }
    // lane: query m = 16 blk + r, keys n0 + i of tile t, n0 = 128 kc + 32 wave + 16 t + 4 g
    const float s = w.scal[2 * pair];
    float* zws = w.zws + (int64_t)pair * 2 * B * w.Bp128;
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n0 = 128 * kc + 32 * wave + 16 * t + 4 * g;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + i;
            const float z = (m < B && n < B) ? s * acc[t][i] : -INFINITY;
            acc[t][i] = z;
            mx = fmaxf(mx, z);
            if (side == 0 && m == n && m < B) w.diag[(int64_t)pair * B + m] = z;
        }
        if (m < B) *(f32x4*)(zws + ((int64_t)side * B + m) * w.Bp128 + n0) = acc[t];
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float ms = mx == -INFINITY ? 0.f : mx;
    float se = 0.f, sw = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float z = acc[t][i];
            const float e = __expf(z - ms);
            se += e;
            sw += z == -INFINITY ? 0.f : e * z;
        }
    se += __shfl_xor(se, 16, 64); se += __shfl_xor(se, 32, 64);
    sw += __shfl_xor(sw, 16, 64); sw += __shfl_xor(sw, 32, 64);
    if (g == 0) { red[wave][0][r] = mx; red[wave][1][r] = se; red[wave][2][r] = sw; }
    __syncthreads();
    if (threadIdx.x < 16 && m < B) {        // the four waves' triples of query r, in a fixed order
        float fm = -INFINITY;
        for (int q = 0; q < 4; ++q) fm = fmaxf(fm, red[q][0][r]);
        float fe = 0.f, fw = 0.f;
        for (int q = 0; q < 4; ++q) {
            const float pm = red[q][0][r];
            if (pm == -INFINITY) continue;
            const float f = __expf(pm - fm);
            fe += red[q][1][r] * f;
            fw += red[q][2][r] * f;
        }
        const int64_t o = (((int64_t)pair * 2 + side) * w.KC + kc) * B + m;
        w.pmax[o] = fm; w.psum[o] = fe; w.pwz[o] = fw;
    }
}

// the chunks' triples of index i on side sd of a pair -> (log-sum-exp, sum exp * z / sum exp); fixed order
__device__ __forceinline__ void ncem_merge(const MultiWs& w, int B, int pair, int sd, int i, float* lse, float* ez) {
    const int64_t base = ((int64_t)pair * 2 + sd) * w.KC;
    float fm = -INFINITY;
    for (int c = 0; c < w.KC; ++c) fm = fmaxf(fm, w.pmax[(base + c) * B + i]);
    float fe = 0.f, fw = 0.f;
    for (int c = 0; c < w.KC; ++c) {
        const int64_t o = (base + c) * B + i;
        const float pm = w.pmax[o];
        if (pm == -INFINITY) continue;
        const float f = __expf(pm - fm);
        fe += w.psum[o] * f;
        fw += w.pwz[o] * f;
    }
    *lse = fm + __logf(fe);
    *ez = fw / fe;
}

template <int E, int CPW>          // CPW: 16-column tiles per wave; blockIdx.z picks the workgroup's 64 CPW columns
__global__ __launch_bounds__(256) void ncem_grad_kernel(MultiWs w, int B, int row0, int nrows, float gscale, float* __restrict__ loss,
                                                        float* __restrict__ dls) {
    __shared__ float lse_o[ROWS_MAX_B];         // log-sum-exp of the OTHER side, per key
    __shared__ float lse_q[16];
    __shared__ float red[2][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int blk = blockIdx.x, op = blockIdx.y, col0 = blockIdx.z * (64 * CPW) + 16 * CPW * wave;
    float* dx = pick(w.dx, op);
    const bool in_strip = dx != nullptr && 16 * blk < row0 + nrows && 16 * blk + 16 > row0;
    const bool sums = blk == 0 && blockIdx.z == 0;
    if (!sums && !in_strip) return;
    const int m = 16 * blk + r;             // lane (r, g): query m as the B-operand column, keys k0 + 8 g .. + 7 as its K slots
    f32x4 acc[CPW];
#pragma unroll
    for (int ct = 0; ct < CPW; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int pair = 0; pair < w.npair; ++pair) {            // ascending k: the order of the sum
        const int a = pick(w.pa, pair), b = pick(w.pb, pair);
        if (a != op && b != op) continue;
        const int side = a == op ? 0 : 1, other = a == op ? b : a;
        __syncthreads();                    // the previous pair's readers of lse_o / lse_q / red are done
        float lsum = 0.f, esum = 0.f;
        const float* diag = w.diag + (int64_t)pair * B;
        for (int n = threadIdx.x; n < B; n += 256) {
            float l, e;
            ncem_merge(w, B, pair, side ^ 1, n, &l, &e);
            lse_o[n] = l;
            const float d = diag[n];
            lsum += l - d;
            esum += e - d;
        }
        if (threadIdx.x < 16 && 16 * blk + (int)threadIdx.x < B) {
            float l, e;
            ncem_merge(w, B, pair, side, 16 * blk + threadIdx.x, &l, &e);
            lse_q[threadIdx.x] = l;
        }
        if (sums) {         // this operand's first workgroup owns the other side's share of the pair's loss and d logit_scale
            red[0][threadIdx.x] = lsum; red[1][threadIdx.x] = esum;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                atomicAdd(w.accum + 2 * pair, red[0][0]);          // two terms per pair: a + b = b + a, the order of arrival does not show
                atomicAdd(w.accum + 2 * pair + 1, red[1][0]);
                __threadfence();
                if (atomicAdd((unsigned int*)(w.accum + 2 * MAXN), 1u) == 2u * (unsigned)w.npair - 1u) {      // the last of all
                    __threadfence();
                    float tot = 0.f;
                    for (int k = 0; k < w.npair; ++k) {
                        const float la = atomicAdd(w.accum + 2 * k, 0.f), lb = atomicAdd(w.accum + 2 * k + 1, 0.f);
                        const float lk = la / (float)B, wk = pick(w.wt, k);
                        loss[k] = lk;
                        tot += wk * lk;
                        if (dls != nullptr) dls[k] = w.scal[2 * k + 1] != 0.f ? 0.f : lb * gscale / (float)B * wk;
                    }
                    loss[w.npair] = tot;
                }
            }
        }
        __syncthreads();
        if (!in_strip) continue;
        const float lq = lse_q[r];
        const float s = w.scal[2 * pair], kf = gscale / (float)B * s * pick(w.wt, pair);
        const float* zrow = w.zws + (((int64_t)pair * 2 + side) * B + (m < B ? m : B - 1)) * w.Bp128 + 8 * g;
        const bf16_t* xt = w.xt + ((int64_t)other * E + col0 + r) * w.Bp32 + 8 * g;       // rows = this wave's columns
        const int nsteps = w.Bp32 / 32;
#pragma unroll 4
        for (int ks = 0; ks < nsteps; ++ks) {
            const int k0 = 32 * ks;
            bf16x8 xf[CPW];
#pragma unroll
            for (int ct = 0; ct < CPW; ++ct) xf[ct] = *(const bf16x8*)(xt + (int64_t)16 * ct * w.Bp32 + k0);
            const f32x4 z0 = *(const f32x4*)(zrow + k0), z1 = *(const f32x4*)(zrow + k0 + 4);
            bf16x8 bd;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int n = k0 + 8 * g + e;
                const float z = e < 4 ? z0[e] : z1[e - 4];
                float d = 0.f;
                if (m < B && n < B) d = (__expf(z - lq) + __expf(z - lse_o[n]) - (m == n ? 2.f : 0.f)) * kf;
                bd[e] = (bf16_t)d;
            }
#pragma unroll
            for (int ct = 0; ct < CPW; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[ct], bd, acc[ct], 0, 0, 0);
        }
    }
    if (in_strip && m >= row0 && m < row0 + nrows && m < B) {
        float* orow = dx + (int64_t)(m - row0) * E + col0 + 4 * g;
#pragma unroll
        for (int ct = 0; ct < CPW; ++ct) *(f32x4*)(orow + 16 * ct) = acc[ct];
    }
}

// sequential path: dx (+)= w * tmp for the two operands of a pair (a NULL dx is skipped), n % 4 == 0
__global__ __launch_bounds__(256) void ncem_axpy_kernel(float* __restrict__ d0, const float* __restrict__ t0, int first0,
                                                        float* __restrict__ d1, const float* __restrict__ t1, int first1, float wk, int64_t n4) {
    float* d = blockIdx.y == 0 ? d0 : d1;
    const float* t = blockIdx.y == 0 ? t0 : t1;
    const int first = blockIdx.y == 0 ? first0 : first1;
    if (d == nullptr) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 v = ((const f32x4*)t)[i] * wk;
        ((f32x4*)d)[i] = first ? v : ((f32x4*)d)[i] + v;
    }
}

__global__ void ncem_finish_kernel(MultiWs w, const float* __restrict__ lt, const float* __restrict__ dt, float* __restrict__ loss,
                                   float* __restrict__ dls) {
    if (threadIdx.x != 0) return;
    float tot = 0.f;
    for (int k = 0; k < w.npair; ++k) {
        const float wk = pick(w.wt, k);
        loss[k] = lt[k];
        tot += wk * lt[k];
        if (dls != nullptr) dls[k] = dt[k] * wk;
    }
    loss[w.npair] = tot;
}

bool fused_path(int64_t B, int64_t E) {
    const char* env = getenv("VIPANT_NCE_MULTI_FUSED");        // =0: every shape through the single-pair launches (A/B timing)
    return B <= ROWS_MAX_B && E == ROWS_E && !(env && env[0] == '0');
}

// sequential path: [single-pair workspace | two gradient temporaries [nrows, E] | loss and d logit_scale temporaries].  A pair whose
// call produces gradients may take the single-pair strip form and a pair that produces none takes the full form, so the
// single-pair part holds the larger of the two: the size does not depend on which operands ask for a gradient.
size_t single_bytes(int64_t B, int64_t E, int64_t nrows) {
    const size_t full = vipant_infonce_workspace_bytes(B, E);
    const size_t strip = nrows > 0 ? vipant_infonce_strip_workspace_bytes(B, E, nrows) : 0;
    return full > strip ? full : strip;
}
size_t seq_bytes(int64_t B, int64_t E, int64_t nrows) {
    return align256(single_bytes(B, E, nrows)) + 2 * align256((size_t)nrows * E * 4) + 256;
}

}  // namespace

extern "C" size_t vipant_infonce_multi_workspace_bytes(int64_t B, int64_t E, int32_t nop, int32_t npair, int64_t nrows) {
    if (B <= 0 || E <= 0 || nop < 1 || nop > MAXN || npair < 1 || npair > MAXN || nrows < 0) return 0;
    return fused_path(B, E) ? carve(nullptr, B, E, nop, npair).total : seq_bytes(B, E, nrows);
}

extern "C" int32_t vipant_infonce_multi_fwd_bwd(const float* const* x, int32_t nop, const int32_t* pair_a, const int32_t* pair_b,
                                                int32_t npair, const float* logit_scale, const float* scale_max, const float* weight,
                                                float* loss, float* const* dx, float* dlogit_scale, float grad_scale, int64_t B,
                                                int64_t E, int64_t row0, int64_t nrows, void* workspace, size_t workspace_bytes,
                                                void* stream) {
    VIPANT_REQUIRE(B > 0 && E > 0 && E % 64 == 0, VIPANT_EBADSHAPE, "infonce_multi: need E %% 64 == 0 (B=%ld E=%ld)", (long)B, (long)E);
    VIPANT_REQUIRE(nop >= 1 && nop <= MAXN && npair >= 1 && npair <= MAXN, VIPANT_EBADSHAPE,
                   "infonce_multi: 1 to %d operands and pairs (nop=%d npair=%d)", MAXN, (int)nop, (int)npair);
    VIPANT_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= B, VIPANT_EBADSHAPE,
                   "infonce_multi: bad row slice [%ld, %ld) of %ld", (long)row0, (long)(row0 + nrows), (long)B);
    VIPANT_REQUIRE(x != nullptr && pair_a != nullptr && pair_b != nullptr && logit_scale != nullptr && scale_max != nullptr &&
                   weight != nullptr && loss != nullptr, VIPANT_EBADSHAPE, "infonce_multi: a required table is NULL");
    bool used[MAXN] = {}, any_dx = false;
    for (int k = 0; k < npair; ++k) {
        VIPANT_REQUIRE(pair_a[k] >= 0 && pair_a[k] < nop && pair_b[k] >= 0 && pair_b[k] < nop, VIPANT_EBADSHAPE,
                       "infonce_multi: pair %d = (%d, %d) names an operand out of range [0, %d)", k, (int)pair_a[k], (int)pair_b[k], (int)nop);
        VIPANT_REQUIRE(pair_a[k] != pair_b[k], VIPANT_EBADSHAPE, "infonce_multi: pair %d scores operand %d against itself", k, (int)pair_a[k]);
        used[pair_a[k]] = used[pair_b[k]] = true;
    }
    for (int i = 0; i < nop; ++i) {
        VIPANT_REQUIRE(x[i] != nullptr, VIPANT_EBADSHAPE, "infonce_multi: operand %d is NULL", i);
        const bool wants = dx != nullptr && dx[i] != nullptr;
        VIPANT_REQUIRE(!wants || used[i], VIPANT_EBADSHAPE, "infonce_multi: operand %d wants a gradient but is in no pair", i);
        any_dx = any_dx || wants;
    }
    const bool want = any_dx && nrows > 0;
    const bool fused = fused_path(B, E);
    MultiWs w = carve((char*)workspace, B, E, nop, npair);
    const int64_t trows = want ? nrows : 0;          // a forward-only call has no gradient temporaries: the nrows = 0 size is enough
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= (fused ? w.total : seq_bytes(B, E, trows)), VIPANT_ENOWORKSPACE,
                   "infonce_multi: workspace too small");
    VIPANT_REQUIRE((uintptr_t)workspace % 256 == 0, VIPANT_EALIGN, "infonce_multi: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < MAXN; ++i) {
        w.x[i] = i < nop ? x[i] : nullptr;
        w.dx[i] = (i < nop && want && dx[i] != nullptr) ? dx[i] : nullptr;
        w.pa[i] = i < npair ? pair_a[i] : 0;
        w.pb[i] = i < npair ? pair_b[i] : 0;
        w.smax[i] = i < npair ? scale_max[i] : 0.f;
        w.wt[i] = i < npair ? weight[i] : 0.f;
    }
    if (fused) {
        int64_t pb = ceil_div((int64_t)E * w.Bp32, 256);
        hipLaunchKernelGGL(ncem_prep_kernel, dim3((unsigned)(pb > 512 ? 512 : pb), (unsigned)nop), dim3(256), 0, s, w, logit_scale, (int)B, (int)E);
        VIPANT_LAUNCH_CHECK();
        hipLaunchKernelGGL(ncem_lse_kernel<ROWS_E>, dim3((unsigned)w.KC, (unsigned)ceil_div(B, 16), 2u * (unsigned)npair), dim3(256), 0, s, w, (int)B);
        VIPANT_LAUNCH_CHECK();
        hipLaunchKernelGGL((ncem_grad_kernel<ROWS_E, 2>), dim3((unsigned)ceil_div(B, 16), (unsigned)nop, ROWS_E / 128), dim3(256), 0, s, w, (int)B,
                           (int)row0, (int)nrows, grad_scale, loss, dlogit_scale);
        VIPANT_LAUNCH_CHECK();
        return VIPANT_OK;
    }
    // the pairs one after another through the single-pair launches
    const size_t single = single_bytes(B, E, trows);
    char* base = (char*)workspace;
    float* ta = (float*)(base + align256(single));
    const size_t tmp_bytes = align256((size_t)trows * E * 4);
    float* tb = (float*)((char*)ta + tmp_bytes);
    float* lt = (float*)((char*)tb + tmp_bytes);
    float* dt = lt + 8;
    bool touched[MAXN] = {};
    for (int k = 0; k < npair; ++k) {
        const int a = pair_a[k], b = pair_b[k];
        float* da = w.dx[a];
        float* db = w.dx[b];
        const int32_t e = vipant_infonce_fwd_bwd(x[a], x[b], logit_scale + k, scale_max[k], lt + k, da ? ta : nullptr, db ? tb : nullptr,
                                                 dlogit_scale ? dt + k : nullptr, grad_scale, B, E, row0, nrows, workspace, single, stream);
        if (e != VIPANT_OK) return e;
        if (da == nullptr && db == nullptr) continue;
        const int64_t n4 = nrows * E / 4;
        int64_t blocks = ceil_div(n4, 256);
        hipLaunchKernelGGL(ncem_axpy_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), 2), dim3(256), 0, s, da, ta, touched[a] ? 0 : 1, db, tb,
                           touched[b] ? 0 : 1, weight[k], n4);
        VIPANT_LAUNCH_CHECK();
        if (da) touched[a] = true;
        if (db) touched[b] = true;
    }
    hipLaunchKernelGGL(ncem_finish_kernel, dim3(1), dim3(64), 0, s, w, lt, dt, loss, dlogit_scale);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}
