// Label-aware symmetric InfoNCE (bidirectional multi-positive contrastive loss, the UniCL / SupCon form): every row of the batch that
// shares a group id with row i is a positive of row i, and the soft-max target is uniform over them,
//   s = min(exp(logit_scale), scale_max);  z_ij = s <x1_i, x2_j>;  P_ij = 1 if i == j or groups[i] == groups[j] >= 0, else 0;
//   n_i = sum_j P_ij (P is symmetric: row and column counts agree);
//   loss = (1/B) sum_i [ lse_j z_ij - (1/n_i) sum_j P_ij z_ij ] + (1/B) sum_j [ lse_i z_ij - (1/n_j) sum_i P_ij z_ij ];
//   G_ij = ( exp(z_ij - rlse_i) + exp(z_ij - clse_j) - 2 P_ij / n_i ) / B;  dx1 = s G x2;  dx2 = s G^T x1;
//   dlogit_scale = sum_ij G_ij z_ij  (0 where the clamp is active).
// groups == NULL (or all ids distinct, or all negative) is P = I: CELossHead's loss.
// A normaliser couples the pairs of a row and of a column, so one walk of the pair matrix cannot finish (the sigmoid loss can): TWO
// walks around sigmoid_loss.hip's register scheme, and still nothing B x B or nrows x B reaches HBM at any batch size.
//
// gfx950 design (four launches):
//   prep   64 x 64 tiles of both operands: the bf16 split [hi | lo] of every row ([B][2E], K-contiguous: the logit product), through an
//          LDS image of the tile the transposed bf16 copy [E][Bp32] (zero beyond B: the gradient product, whose K runs over the batch),
//          the group ids as int32 [Bp32] (-1 = "no label" for NULL groups and beyond B, so the walks never see a NULL), and s and the
//          clamp flag as device scalars.
//   stats  workgroup = (16 "query" rows, side), over ALL B rows on both sides: the gradient of a strip needs every column's clse.
//          The queries' [hi | lo] rows sit in LDS (padded by 16 B per row); the four waves split the 32-key steps w, w + 4, ...  Per
//          step a wave forms two 16 x 16 logit tiles with v_mfma_f32_16x16x32_bf16 -- keys as the A operand straight from global memory,
//          three terms hi.hi + (hi.lo + lo.hi): logits at fp32 grade, needed at EVERY positive pair, where exp(z - lse) cancels against
//          1 / n and identical prompt rows make the logits equal to the diagonal's -- and each lane folds its eight (query lane & 15,
//          key) logits into an online (max, sum exp, sum exp z) triple, sum P z and n; the step's key ids are one 16-byte load per tile,
//          compared in registers.  The triples of a query merge across its four lane groups and the four waves through LDS in a fixed
//          order.  Outputs: rlse / clse [B], n [B], and per workgroup the partial sums of the loss (lse - sum P z / n) and of
//          sum G z (sum exp z / sum exp - sum P z / n).
//   grad   workgroup = (16 query rows of the STRIP, side, E-chunk), sig_walk_kernel's shape: the logits are recomputed, the lane forms G
//          for its eight pairs from its query's lse and 1 / n and the step's 32 key-side lse and ids, rounds it once to bf16 and uses
//          it directly as the B operand of dx^T[16 columns x 16 queries] += x_key^T . G^T against the transposed copy read in the same
//          key order: G never leaves the registers.  Side 1 swaps the operands and the two lse vectors.  E-chunks of <= 512 columns.
//   fold   one workgroup adds the stats partials in a fixed order (fp64) and writes loss and dlogit_scale.
// Strip convention (row0, nrows): InfoNCEFn's -- loss and dlogit_scale are the full-batch values on every caller, dx1 / dx2 the
// rows [row0, row0 + nrows), pre-multiplied by grad_scale.
// Deterministic: no atomics; every sum has a fixed order.  exp / log in fp32.
#include "common.h"

namespace {

struct LnceWs {     // carved out of the caller's workspace; every offset 256-B aligned
    bf16_t *xs1, *xs2;      // [B][2E]: hi | lo
    bf16_t *xt1, *xt2;      // [E][Bp]: bf16(x)^T, columns B .. Bp zero
    int* gid;               // [Bp]: group id, -1 beyond B and for NULL groups
    float *rlse, *clse;     // [Bp]: log-sum-exp of the rows / columns of z (B live)
    float* cnt;             // [Bp]: n (B live)
    float* scal;            // s, clamp flag
    float* part;            // [nblk][2 sides][2]: loss and sum G z terms of a block of 16 queries
    int Bp, nblk;
    size_t total;
};

size_t lnce_align256(size_t x) { return (x + 255) & ~(size_t)255; }

LnceWs lnce_carve(char* base, int64_t B, int64_t E) {
    LnceWs w;
    w.Bp = (int)((B + 31) / 32 * 32);
    w.nblk = (int)ceil_div(B, 16);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += lnce_align256(bytes); return p; };
    w.xs1 = (bf16_t*)take((size_t)B * 2 * E * 2);
    w.xs2 = (bf16_t*)take((size_t)B * 2 * E * 2);
    w.xt1 = (bf16_t*)take((size_t)E * w.Bp * 2);
    w.xt2 = (bf16_t*)take((size_t)E * w.Bp * 2);
    w.gid = (int*)take((size_t)w.Bp * 4);
    w.rlse = (float*)take((size_t)w.Bp * 4);
    w.clse = (float*)take((size_t)w.Bp * 4);
    w.cnt = (float*)take((size_t)w.Bp * 4);
    w.scal = (float*)take(256);
    w.part = (float*)take((size_t)w.nblk * 4 * 4);
    w.total = off;
    return w;
}

// grid (E / 64, ceil(Bp / 64), 2 operands)
__global__ __launch_bounds__(256) void lnce_prep_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                        const int32_t* __restrict__ groups, const float* __restrict__ logit_scale,
                                                        float scale_max, LnceWs w, int B, int E) {
    __shared__ bf16_t tile[64][66];
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
        const float raw = expf(logit_scale[0]);
        const bool clamped = scale_max > 0.f && raw > scale_max;
        w.scal[0] = clamped ? scale_max : raw;
        w.scal[1] = clamped ? 1.f : 0.f;
    }
    const int tr = blockIdx.y * 64, tc = blockIdx.x * 64;
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x < 64) {       // the ids of this tile's rows
        const int gr = tr + threadIdx.x;
        if (gr < w.Bp) w.gid[gr] = (groups != nullptr && gr < B) ? groups[gr] : -1;
    }
    const float* src = blockIdx.z == 0 ? x1 : x2;
    bf16_t* xs = blockIdx.z == 0 ? w.xs1 : w.xs2;
    bf16_t* xt = blockIdx.z == 0 ? w.xt1 : w.xt2;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int gr = tr + r, gc = tc + tx;
        bf16_t hi = (bf16_t)0.0f;
        if (gr < B) {
            const float v = src[(int64_t)gr * E + gc];
            hi = (bf16_t)v;
            xs[(int64_t)gr * 2 * E + gc] = hi;
            xs[(int64_t)gr * 2 * E + E + gc] = (bf16_t)(v - (float)hi);
        }
        tile[r][tx] = hi;
    }
    __syncthreads();
    for (int c = ty; c < 64; c += 4) {
        const int gc = tc + c, gr = tr + tx;
        if (gr < w.Bp) xt[(int64_t)gc * w.Bp + gr] = tile[tx][c];
    }
}

constexpr int LNCE_QPAD = 16;       // bytes added to a query row in LDS: a fragment read touches every bank once

// the 16 queries' [hi | lo] rows (rows q0 .. q0 + 15 of xq, clamped to the batch) -> LDS, 16 bytes per thread and turn
__device__ __forceinline__ void lnce_stage_queries(char* smem, const bf16_t* __restrict__ xq, int q0, int B, int E) {
    const int qstride = 4 * E + LNCE_QPAD;
    for (int u = threadIdx.x; u < 4 * E; u += 256) {
        const int row = u / (E / 4), cu = u % (E / 4);
        int q = q0 + row;
        q = q < B ? q : B - 1;
        *(u32x4*)(smem + row * qstride + cu * 16) = *(const u32x4*)(xq + (int64_t)q * 2 * E + cu * 8);
    }
}

// <x_query, x_key> of one 32-key step at fp32 grade: lane (r = lane & 15, g = lane >> 4) ends up with query r against the keys
// k0 + 16 t + 4 g + i in d[4 t + i].  Keys are the A operand (row = lane & 15) straight from global memory, queries the B operand
// from LDS; hi.hi and (hi.lo + lo.hi) in two accumulators per tile: four independent MFMA chains.
__device__ __forceinline__ void lnce_logits(const char* qrow, const bf16_t* __restrict__ xk, int k0, int r, int g, int B, int E, float* d) {
    const bf16_t* kp[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int n = k0 + 16 * t + r;
        kp[t] = xk + (int64_t)(n < B ? n : B - 1) * 2 * E + 8 * g;
    }
    f32x4 zh[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 zx[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int esteps = E / 32;
    for (int es = 0; es < esteps; ++es) {
        const bf16x8 qh = *(const bf16x8*)(qrow + 64 * es), ql = *(const bf16x8*)(qrow + 2 * E + 64 * es);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bf16x8 kh = *(const bf16x8*)(kp[t] + 32 * es), kl = *(const bf16x8*)(kp[t] + E + 32 * es);
            zh[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh, zh[t], 0, 0, 0);
            zx[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql, zx[t], 0, 0, 0);
            zx[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qh, zx[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) d[4 * t + i] = zh[t][i] + zx[t][i];
}

// grid (ceil(B / 16), 2 sides); dynamic LDS: the queries' rows
__global__ __launch_bounds__(256) void lnce_stats_kernel(LnceWs w, int B, int E) {
    extern __shared__ __attribute__((aligned(16))) char lnce_smem[];
    __shared__ float red[4][4][5][16];          // [wave][lane group][max, sum exp, sum exp z, sum P z, n][query]
    __shared__ float term[2][16];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 15, g = lane >> 4;
    const int blk = blockIdx.x, side = blockIdx.y;
    const bf16_t* xq = side == 0 ? w.xs1 : w.xs2;       // queries
    const bf16_t* xk = side == 0 ? w.xs2 : w.xs1;       // keys
    lnce_stage_queries(lnce_smem, xq, 16 * blk, B, E);
    __syncthreads();
    const int m = 16 * blk + r;                         // this lane's query
    const int gq = w.gid[m < B ? m : B - 1];
    const float s = w.scal[0];
    const char* qrow = lnce_smem + r * (4 * E + LNCE_QPAD) + 16 * g;
    float mx = -INFINITY, se = 0.f, sw = 0.f, pz = 0.f, pn = 0.f;
    const int nsteps = w.Bp / 32;
    for (int ks = wave; ks < nsteps; ks += 4) {
        const int k0 = 32 * ks;
        float d[8];
        lnce_logits(qrow, xk, k0, r, g, B, E, d);
        float z[8], mx8 = -INFINITY;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n0 = k0 + 16 * t + 4 * g;
            const v4i32_t gk = *(const v4i32_t*)(w.gid + n0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + i;
                const bool live = n < B;
                z[4 * t + i] = live ? s * d[4 * t + i] : -INFINITY;
                mx8 = fmaxf(mx8, z[4 * t + i]);
                if (live && (n == m || (gq >= 0 && gk[i] == gq))) { pz += z[4 * t + i]; pn += 1.f; }
            }
        }
        if (mx8 > -INFINITY) {          // at least one live key: the online soft-max step
            const float nm = fmaxf(mx, mx8), f = expf(mx - nm);        // mx == -inf: f = 0
            se *= f; sw *= f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (z[j] > -INFINITY) {
                    const float e = expf(z[j] - nm);
                    se += e;
                    sw = __builtin_fmaf(e, z[j], sw);
                }
            mx = nm;
        }
    }
    red[wave][g][0][r] = mx; red[wave][g][1][r] = se; red[wave][g][2][r] = sw; red[wave][g][3][r] = pz; red[wave][g][4][r] = pn;
    __syncthreads();
    if (threadIdx.x < 16) {             // query r: its 16 partial triples, waves outer, lane groups inner
        const float* p = &red[0][0][0][0];
        float fm = -INFINITY;
        for (int q = 0; q < 16; ++q) fm = fmaxf(fm, p[(q * 5 + 0) * 16 + r]);
        float fe = 0.f, fw = 0.f, fp = 0.f, fn = 0.f;
        for (int q = 0; q < 16; ++q) {
            const float pm = p[(q * 5 + 0) * 16 + r];
            fp += p[(q * 5 + 3) * 16 + r];
            fn += p[(q * 5 + 4) * 16 + r];
            if (pm == -INFINITY) continue;
            const float f = expf(pm - fm);
            fe = __builtin_fmaf(p[(q * 5 + 1) * 16 + r], f, fe);
            fw = __builtin_fmaf(p[(q * 5 + 2) * 16 + r], f, fw);
        }
        float tl = 0.f, tg = 0.f;
        if (m < B) {
            const float lse = fm + logf(fe), pos = fp / fn;     // n >= 1: the query's own pair
            (side == 0 ? w.rlse : w.clse)[m] = lse;
            if (side == 0) w.cnt[m] = fn;
            tl = lse - pos;
            tg = fw / fe - pos;
        }
        term[0][r] = tl; term[1][r] = tg;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        float a = 0.f;
        for (int q = 0; q < 16; ++q) a += term[threadIdx.x][q];
        w.part[(2 * blk + side) * 2 + threadIdx.x] = a;
    }
}

template <int NCT>          // 64-column groups of an E-chunk: a wave's accumulators are [16 queries x 64 NCT columns]
__global__ __launch_bounds__(256) void lnce_grad_kernel(LnceWs w, int B, int E, float* __restrict__ dx1, float* __restrict__ dx2, int row0,
                                                        int nrows, float gscale) {
    extern __shared__ __attribute__((aligned(16))) char lnce_smem[];
    constexpr int NT = 4 * NCT;                 // 16-column tiles
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 15, g = lane >> 4;
    const int blk = blockIdx.x, side = blockIdx.y, col0 = blockIdx.z * (64 * NCT);
    float* dx = side == 0 ? dx1 : dx2;
    if (dx == nullptr) return;
    const bf16_t* xq = side == 0 ? w.xs1 : w.xs2;       // queries
    const bf16_t* xk = side == 0 ? w.xs2 : w.xs1;       // keys, K-contiguous (the logit product)
    const bf16_t* xt = side == 0 ? w.xt2 : w.xt1;       // keys, transposed (the gradient product)
    const float* lse_q = side == 0 ? w.rlse : w.clse;
    const float* lse_k = side == 0 ? w.clse : w.rlse;
    lnce_stage_queries(lnce_smem, xq, row0 + 16 * blk, B, E);
    __syncthreads();
    const int ml = 16 * blk + r, m = row0 + ml;         // this lane's query: row inside the strip, row of the batch
    const bool qlive = ml < nrows;
    const int mc = m < B ? m : B - 1;
    const int gq = w.gid[mc];
    const float lq = lse_q[mc], pw = 2.0f / w.cnt[mc];  // P_ij / n_i: n is the same on both ends of a positive pair
    const float s = w.scal[0], inv_b = 1.0f / (float)B;
    const char* qrow = lnce_smem + r * (4 * E + LNCE_QPAD) + 16 * g;
    f32x4 acc[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nsteps = w.Bp / 32;
    for (int ks = wave; ks < nsteps; ks += 4) {
        const int k0 = 32 * ks;
        // 1. logits, as the stats walk formed them
        float d[8];
        lnce_logits(qrow, xk, k0, r, g, B, E, d);
        // 2. gradient coefficients: lane = query r, keys k0 + 16 t + 4 g + i
        bf16x8 bd;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n0 = k0 + 16 * t + 4 * g;
            const v4i32_t gk = *(const v4i32_t*)(w.gid + n0);
            const f32x4 lk = *(const f32x4*)(lse_k + n0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + i;
                const float z = s * d[4 * t + i];
                const bool pos = n == m || (gq >= 0 && gk[i] == gq);
                float gv = 0.f;
                if (qlive && n < B) gv = (expf(z - lq) + expf(z - lk[i]) - (pos ? pw : 0.f)) * inv_b;
                bd[4 * t + i] = (bf16_t)gv;
            }
        }
        // 3. dx^T[column tile x queries] += x_key^T[columns x these 32 keys] . G^T, the keys in the order the lanes hold G
        const bf16_t* xp = xt + (int64_t)(col0 + r) * w.Bp + k0 + 4 * g;
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            if (col0 + 16 * ct < E) {
                const u32x2 a0 = *(const u32x2*)(xp + (int64_t)16 * ct * w.Bp), a1 = *(const u32x2*)(xp + (int64_t)16 * ct * w.Bp + 16);
                const u32x4 a = u32x4{a0[0], a0[1], a1[0], a1[1]};
                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), bd, acc[ct], 0, 0, 0);
            }
        }
    }
    __syncthreads();                // every wave is done with the queries in LDS
    // the four waves' partial accumulators: (w0 + w2) + (w1 + w3)
    f32x4* buf = (f32x4*)lnce_smem;
    if (wave >= 2) {
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) buf[((wave - 2) * NT + ct) * 64 + lane] = acc[ct];
    }
    __syncthreads();
    if (wave < 2) {
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc[ct] += buf[(wave * NT + ct) * 64 + lane];
    }
    __syncthreads();
    if (wave == 1) {
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) buf[ct * 64 + lane] = acc[ct];
    }
    __syncthreads();
    if (wave == 0 && qlive) {       // lane: query r, columns col0 + 16 ct + 4 g .. + 3
        const float k = s * gscale;
        float* orow = dx + (int64_t)ml * E + col0 + 4 * g;
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
            if (col0 + 16 * ct < E) *(f32x4*)(orow + 16 * ct) = (acc[ct] + buf[ct * 64 + lane]) * k;
    }
}

__global__ __launch_bounds__(256) void lnce_fold_kernel(LnceWs w, int B, float gscale, float* __restrict__ loss, float* __restrict__ dls) {
    __shared__ double red[2][256];
    double a[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < 2 * w.nblk; i += 256)
        for (int q = 0; q < 2; ++q) a[q] += (double)w.part[2 * i + q];
    for (int q = 0; q < 2; ++q) red[q][threadIdx.x] = a[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int q = 0; q < 2; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double inv_b = 1.0 / (double)B;
        loss[0] = (float)(red[0][0] * inv_b);
        if (dls != nullptr) dls[0] = w.scal[1] != 0.f ? 0.f : (float)(red[1][0] * inv_b * (double)gscale);
    }
}

bool lnce_shape_ok(int64_t B, int64_t E) { return B >= 1 && B < (1ll << 30) && E % 64 == 0 && E >= 64 && E <= 1024; }

int lnce_query_bytes(int64_t E) { return 16 * (int)(4 * E + LNCE_QPAD); }

// launch == false: only raises the kernel's dynamic-LDS limit on this device (done before the call's first launch, so that a failure
// there leaves nothing written); launch == true: the gradient walk
template <int NCT>
int32_t lnce_grad(bool launch, const LnceWs& w, int64_t B, int64_t E, float* dx1, float* dx2, int64_t row0, int64_t nrows, float gscale,
                  hipStream_t s) {
    const int chunks = (int)ceil_div(E, 64 * NCT);
    const int qbytes = lnce_query_bytes(E), rbytes = 2 * 4 * NCT * 64 * 16;
    const int lds = qbytes > rbytes ? qbytes : rbytes;
    if (!launch) {
        static DeviceMax most;
        if (raise_on_device(most, lds)) {
            VIPANT_HIP_TRY(hipFuncSetAttribute((const void*)lnce_grad_kernel<NCT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            raised_on_device(most, lds);
        }
        return VIPANT_OK;
    }
    hipLaunchKernelGGL(lnce_grad_kernel<NCT>, dim3((unsigned)ceil_div(nrows, 16), 2, (unsigned)chunks), dim3(256), lds, s, w, (int)B, (int)E,
                       dx1, dx2, (int)row0, (int)nrows, gscale);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

int32_t lnce_grad_any(bool launch, const LnceWs& w, int64_t B, int64_t E, float* dx1, float* dx2, int64_t row0, int64_t nrows, float gscale,
                      hipStream_t s) {
    // E <= 512: one chunk of E columns; above: two chunks of ceil(E / 128) * 64
    switch ((int)(E <= 512 ? E / 64 : ceil_div(E, 128))) {
        case 1: return lnce_grad<1>(launch, w, B, E, dx1, dx2, row0, nrows, gscale, s);
        case 2: return lnce_grad<2>(launch, w, B, E, dx1, dx2, row0, nrows, gscale, s);
        case 3: return lnce_grad<3>(launch, w, B, E, dx1, dx2, row0, nrows, gscale, s);
        case 4: return lnce_grad<4>(launch, w, B, E, dx1, dx2, row0, nrows, gscale, s);
        case 5: return lnce_grad<5>(launch, w, B, E, dx1, dx2, row0, nrows, gscale, s);
        case 6: return lnce_grad<6>(launch, w, B, E, dx1, dx2, row0, nrows, gscale, s);
        case 7: return lnce_grad<7>(launch, w, B, E, dx1, dx2, row0, nrows, gscale, s);
        case 8: return lnce_grad<8>(launch, w, B, E, dx1, dx2, row0, nrows, gscale, s);
    }
    return VIPANT_EBADSHAPE;
}

}  // namespace

extern "C" size_t vipant_label_nce_workspace_bytes(int64_t B, int64_t E, int64_t nrows) {
    return lnce_shape_ok(B, E) && nrows >= 0 && nrows <= B ? lnce_carve(nullptr, B, E).total : 0;
}

extern "C" int32_t vipant_label_nce_fwd_bwd(const float* x1, const float* x2, const int32_t* groups, const float* logit_scale,
                                            float scale_max, float* loss, float* dx1, float* dx2, float* dlogit_scale, float grad_scale,
                                            int64_t B, int64_t E, int64_t row0, int64_t nrows, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    VIPANT_REQUIRE(lnce_shape_ok(B, E), VIPANT_EBADSHAPE, "label_nce: need B >= 1, E %% 64 == 0 and 64 <= E <= 1024 (B=%ld E=%ld)", (long)B,
                   (long)E);
    VIPANT_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= B, VIPANT_EBADSHAPE, "label_nce: bad row slice [%ld, %ld) of %ld", (long)row0,
                   (long)(row0 + nrows), (long)B);
    VIPANT_REQUIRE(x1 != nullptr && x2 != nullptr && logit_scale != nullptr && loss != nullptr, VIPANT_EBADSHAPE,
                   "label_nce: x1, x2, logit_scale and loss are required");
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= vipant_label_nce_workspace_bytes(B, E, nrows), VIPANT_ENOWORKSPACE,
                   "label_nce: workspace too small (%zu bytes needed, %zu given)", vipant_label_nce_workspace_bytes(B, E, nrows),
                   workspace_bytes);
    VIPANT_REQUIRE((uintptr_t)workspace % 256 == 0, VIPANT_EALIGN, "label_nce: workspace must be 256-byte aligned");
    VIPANT_REQUIRE((uintptr_t)dx1 % 16 == 0 && (uintptr_t)dx2 % 16 == 0, VIPANT_EALIGN, "label_nce: dx1 / dx2 must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const LnceWs w = lnce_carve((char*)workspace, B, E);
    const int qbytes = lnce_query_bytes(E);
    const bool grads = (dx1 != nullptr || dx2 != nullptr) && nrows > 0;
    static DeviceMax most;
    if (raise_on_device(most, qbytes)) {        // both walks' LDS limits before the first launch: a failure here leaves nothing written
        VIPANT_HIP_TRY(hipFuncSetAttribute((const void*)lnce_stats_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, qbytes));
        raised_on_device(most, qbytes);
    }
    if (grads) {
        const int32_t rc = lnce_grad_any(false, w, B, E, dx1, dx2, row0, nrows, grad_scale, s);
        if (rc != VIPANT_OK) return rc;
    }
    hipLaunchKernelGGL(lnce_prep_kernel, dim3((unsigned)(E / 64), (unsigned)ceil_div(w.Bp, 64), 2), dim3(256), 0, s, x1, x2, groups,
                       logit_scale, scale_max, w, (int)B, (int)E);
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(lnce_stats_kernel, dim3((unsigned)w.nblk, 2), dim3(256), qbytes, s, w, (int)B, (int)E);
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(lnce_fold_kernel, dim3(1), dim3(256), 0, s, w, (int)B, grad_scale, loss, dlogit_scale);
    VIPANT_LAUNCH_CHECK();
    return grads ? lnce_grad_any(true, w, B, E, dx1, dx2, row0, nrows, grad_scale, s) : VIPANT_OK;
}
