// Pairwise sigmoid contrastive loss (SigLIP): every pair (i, j) of the batch is a binary problem of its own,
//   s = min(exp(logit_scale), scale_max);  z_ij = s <x1_i, x2_j> + logit_bias;  y_ij = +1 on the diagonal, -1 elsewhere;
//   loss = (1/B) sum_ij softplus(-y_ij z_ij);  G_ij = -y_ij sigmoid(-y_ij z_ij) / B;  dx1 = s G x2;  dx2 = s G^T x1;
//   dlogit_bias = sum_ij G_ij;  dlogit_scale = s sum_ij G_ij <x1_i, x2_j>  (0 where the clamp is active).
// No normaliser couples the pairs, so a tile of logits is turned into its loss terms, its gradient coefficients and its share of both
// gradient contractions and then forgotten: ONE walk, nothing B x B (or nrows x B) ever reaches HBM, at every batch size.
//
// gfx950 design (two launches and a one-workgroup fold):
//   prep   one launch, 64 x 64 tiles of both operands: the bf16 split [hi | lo] of every row ([B][2E], K-contiguous: the logit product)
//          and, through an LDS image of the tile, the transposed bf16 copy [E][Bp32] (zero beyond B: the gradient product, whose K runs
//          over the batch), plus s, the clamp flag and the bias as device scalars.
//   walk   workgroup = (16 "query" rows of the strip, side, E-chunk).  Side 0: queries are rows of x1, keys all B rows of x2, the
//          result rows of dx1 (the strip's ROWS of G); side 1 swaps the operands and yields dx2 (the strip's COLUMNS of G): z and y are
//          symmetric under the swap, so it is the same code.  The 16 queries' [hi | lo] rows sit in LDS (padded by 16 B per row: a
//          fragment read touches every bank once) and are shared by the four waves, which split the KEYS: wave w takes the 32-key
//          steps w, w + 4, ...  Per step a wave
//            1. forms two 16 x 16 logit tiles with v_mfma_f32_16x16x32_bf16, keys as the A operand straight from global memory, three
//               terms hi.hi + (hi.lo + lo.hi) in two accumulators each (four independent MFMA chains): logits at fp32 grade, the
//               dropped lo.lo term is below 4e-6 of |x1| |x2|;
//            2. applies softplus / sigmoid in registers (|u| form: exact in both saturated limits) and adds its loss, dlogit_bias and
//               dlogit_scale terms (side 0, chunk 0 only);
//            3. uses the eight bf16 G values it holds -- query lane & 15, keys 4 (lane >> 4) + {0..3} and 16 + 4 (lane >> 4) + {0..3}
//               -- directly as the B operand of dx^T[16 columns x 16 queries] += x_key^T . G^T.  The K slots of an MFMA may hold the 32
//               keys in any order as long as both operands agree, so the A operand is read from the transposed copy in the SAME order
//               (two 8-byte loads per lane) and G never leaves the registers: no LDS round trip, no transposed fragment read.
//          At the end the four waves' partial [16 x chunk] accumulators are added through LDS in the fixed order (w0 + w2) + (w1 + w3).
//   fold   one workgroup adds the per-row-block scalar partials in a fixed order (fp64) and writes loss, dlogit_scale, dlogit_bias.
// The accumulator trade: 16 queries x 512 columns of fp32 are 128 registers per lane, what one wave can keep beside the logit tiles.
// E <= 512 is one chunk; E > 512 runs two chunks of ceil(E / 128) * 64 columns in workgroups of their own, each recomputing its
// logits (the logit product costs 3 E / 32 MFMAs per tile against E / 32 for the gradient: a chunk narrower than 512 would pay
// more for logits than it saves).  Fewer than 16 rows per workgroup cannot be expressed in the 16 x 16 instruction.
// Strip convention (row0, nrows): dx1 / dx2 are the strip's rows; loss, dlogit_scale and dlogit_bias are the sums over the strip's
// ROWS of the pair matrix (i in the strip, all j), normalised by 1/B: the full values when nrows == B, and under replicas the ranks'
// values add up to the full ones (the host reduces them) -- no tile outside the strip's rows and columns is walked.
// Deterministic: no atomics; every sum has a fixed order.  exp / log1p in fp32.
#include "common.h"

namespace {

struct SigWs {      // carved out of the caller's workspace; every offset 256-B aligned
    bf16_t *xs1, *xs2;      // [B][2E]: hi | lo
    bf16_t *xt1, *xt2;      // [E][Bp]: bf16(x)^T, columns B .. Bp zero
    float *scal;            // s, clamp flag, bias
    float *part;            // [nblk][4]: loss, dlogit_bias, dlogit_scale terms of a row block
    int Bp, nblk;
    size_t total;
};

size_t sig_align256(size_t x) { return (x + 255) & ~(size_t)255; }

SigWs sig_carve(char* base, int64_t B, int64_t E, int64_t nrows) {
    SigWs w;
    w.Bp = (int)((B + 31) / 32 * 32);
    w.nblk = (int)ceil_div(nrows, 16);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += sig_align256(bytes); return p; };
    w.xs1 = (bf16_t*)take((size_t)B * 2 * E * 2);
    w.xs2 = (bf16_t*)take((size_t)B * 2 * E * 2);
    w.xt1 = (bf16_t*)take((size_t)E * w.Bp * 2);
    w.xt2 = (bf16_t*)take((size_t)E * w.Bp * 2);
    w.scal = (float*)take(256);
    w.part = (float*)take((size_t)w.nblk * 4 * 4);
    w.total = off;
    return w;
}

// grid (E / 64, ceil(Bp / 64), 2 operands)
__global__ __launch_bounds__(256) void sig_prep_kernel(const float* __restrict__ x1, const float* __restrict__ x2,
                                                       const float* __restrict__ logit_scale, const float* __restrict__ logit_bias,
                                                       float scale_max, SigWs w, int B, int E) {
    __shared__ bf16_t tile[64][66];
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
        const float raw = expf(logit_scale[0]);
        const bool clamped = scale_max > 0.f && raw > scale_max;
        w.scal[0] = clamped ? scale_max : raw;
        w.scal[1] = clamped ? 1.f : 0.f;
        w.scal[2] = logit_bias[0];
    }
    const float* src = blockIdx.z == 0 ? x1 : x2;
    bf16_t* xs = blockIdx.z == 0 ? w.xs1 : w.xs2;
    bf16_t* xt = blockIdx.z == 0 ? w.xt1 : w.xt2;
    const int tr = blockIdx.y * 64, tc = blockIdx.x * 64;
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

constexpr int SIG_QPAD = 16;        // bytes added to a query row in LDS

template <int NCT>          // 64-column groups of an E-chunk: a wave's accumulators are [16 queries x 64 NCT columns]
__global__ __launch_bounds__(256) void sig_walk_kernel(SigWs w, int B, int E, float* __restrict__ dx1, float* __restrict__ dx2, int row0,
                                                       int nrows, float gscale) {
    extern __shared__ __attribute__((aligned(16))) char sig_smem[];
    __shared__ float red[4][3];
    constexpr int NT = 4 * NCT;                 // 16-column tiles
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 15, g = lane >> 4;
    const int blk = blockIdx.x, side = blockIdx.y, col0 = blockIdx.z * (64 * NCT);
    float* dx = side == 0 ? dx1 : dx2;
    const bool sums = side == 0 && blockIdx.z == 0;
    if (dx == nullptr && !sums) return;
    const bf16_t* xq = side == 0 ? w.xs1 : w.xs2;       // queries
    const bf16_t* xk = side == 0 ? w.xs2 : w.xs1;       // keys, K-contiguous (the logit product)
    const bf16_t* xt = side == 0 ? w.xt2 : w.xt1;       // keys, transposed (the gradient product)
    const int qstride = 4 * E + SIG_QPAD;
    // the 16 queries' [hi | lo] rows -> LDS, 16 bytes per thread and turn
    for (int u = threadIdx.x; u < 4 * E; u += 256) {
        const int row = u / (E / 4), cu = u % (E / 4);
        int q = row0 + 16 * blk + row;
        q = q < B ? q : B - 1;
        *(u32x4*)(sig_smem + row * qstride + cu * 16) = *(const u32x4*)(xq + (int64_t)q * 2 * E + cu * 8);
    }
    __syncthreads();
    const int ml = 16 * blk + r, m = row0 + ml;         // this lane's query: row inside the strip, row of the batch
    const bool qlive = ml < nrows;
    const float s = w.scal[0], bias = w.scal[2], inv_b = 1.0f / (float)B;
    const char* qrow = sig_smem + r * qstride + 16 * g;
    f32x4 acc[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f, bsum = 0.f, ssum = 0.f;
    const int nsteps = w.Bp / 32, esteps = E / 32;
    for (int ks = wave; ks < nsteps; ks += 4) {
        const int k0 = 32 * ks;
        // 1. logits: keys (A operand, row = lane & 15) x queries (B operand, column = lane & 15)
        const bf16_t* kp[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int n = k0 + 16 * t + r;
            kp[t] = xk + (int64_t)(n < B ? n : B - 1) * 2 * E + 8 * g;
        }
        f32x4 zh[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        f32x4 zx[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
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
        // 2. loss terms and gradient coefficients: lane = query r, keys k0 + 16 t + 4 g + i
        bf16x8 bd;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = k0 + 16 * t + 4 * g + i;
                const float d = zh[t][i] + zx[t][i];
                const float z = __builtin_fmaf(s, d, bias);
                const bool pos = n == m;
                const float u = pos ? -z : z;               // -y z
                const float au = fabsf(u);
                const float e = expf(-au);                  // in (0, 1]: no overflow, and 0 in the saturated limit
                const float sg = (u >= 0.f ? 1.0f : e) / (1.0f + e);        // sigmoid(u)
                float gv = 0.f;
                if (qlive && n < B) {
                    gv = pos ? -sg : sg;                    // -y sigmoid(-y z)
                    if (sums) {
                        lsum += fmaxf(u, 0.f) + log1pf(e);  // softplus(u)
                        bsum += gv;
                        ssum = __builtin_fmaf(gv, d, ssum);
                    }
                }
                bd[4 * t + i] = (bf16_t)(gv * inv_b);
            }
        // 3. dx^T[column tile x queries] += x_key^T[columns x these 32 keys] . G^T, the keys in the order the lanes hold G
        if (dx != nullptr) {
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
    }
    if (sums) {         // the row block's scalar terms: lanes, then waves, in a fixed order
        lsum = wave_sum(lsum); bsum = wave_sum(bsum); ssum = wave_sum(ssum);
        if (lane == 0) { red[wave][0] = lsum; red[wave][1] = bsum; red[wave][2] = ssum; }
    }
    __syncthreads();                // (also: every wave is done with the queries in LDS)
    if (sums && threadIdx.x < 3) {
        const int q = threadIdx.x;
        w.part[4 * blk + q] = (red[0][q] + red[2][q]) + (red[1][q] + red[3][q]);
    }
    if (dx == nullptr) return;
    // the four waves' partial accumulators: (w0 + w2) + (w1 + w3)
    f32x4* buf = (f32x4*)sig_smem;
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

__global__ __launch_bounds__(256) void sig_fold_kernel(SigWs w, int B, float gscale, float* __restrict__ loss, float* __restrict__ dls,
                                                       float* __restrict__ dlb) {
    __shared__ double red[3][256];
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < w.nblk; i += 256)
        for (int q = 0; q < 3; ++q) a[q] += (double)w.part[4 * i + q];
    for (int q = 0; q < 3; ++q) red[q][threadIdx.x] = a[q];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double inv_b = 1.0 / (double)B;
        loss[0] = (float)(red[0][0] * inv_b);
        if (dlb != nullptr) dlb[0] = (float)(red[1][0] * inv_b * (double)gscale);
        if (dls != nullptr) dls[0] = w.scal[1] != 0.f ? 0.f : (float)(red[2][0] * inv_b * (double)gscale * (double)w.scal[0]);
    }
}

bool sig_shape_ok(int64_t B, int64_t E, int64_t nrows) {
    return B >= 1 && B < (1ll << 30) && E % 64 == 0 && E >= 64 && E <= 1024 && nrows > 0 && nrows <= B;
}

template <int NCT>
int32_t sig_launch_walk(const SigWs& w, int64_t B, int64_t E, float* dx1, float* dx2, int64_t row0, int64_t nrows, float gscale, hipStream_t s) {
    const int chunks = (int)ceil_div(E, 64 * NCT);
    const bool grads = dx1 != nullptr || dx2 != nullptr;
    const int qbytes = 16 * (int)(4 * E + SIG_QPAD), rbytes = grads ? 2 * 4 * NCT * 64 * 16 : 0;
    const int lds = qbytes > rbytes ? qbytes : rbytes;
    static DeviceMax most;
    if (raise_on_device(most, lds)) {
        VIPANT_HIP_TRY(hipFuncSetAttribute((const void*)sig_walk_kernel<NCT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        raised_on_device(most, lds);
    }
    hipLaunchKernelGGL(sig_walk_kernel<NCT>, dim3((unsigned)w.nblk, grads ? 2 : 1, (unsigned)chunks), dim3(256), lds, s, w, (int)B, (int)E, dx1,
                       dx2, (int)row0, (int)nrows, gscale);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

}  // namespace

extern "C" size_t vipant_sigmoid_loss_workspace_bytes(int64_t B, int64_t E, int64_t nrows) {
    return sig_shape_ok(B, E, nrows) ? sig_carve(nullptr, B, E, nrows).total : 0;
}

extern "C" int32_t vipant_sigmoid_loss_fwd_bwd(const float* x1, const float* x2, const float* logit_scale, const float* logit_bias,
                                               float scale_max, float* loss, float* dx1, float* dx2, float* dlogit_scale,
                                               float* dlogit_bias, float grad_scale, int64_t B, int64_t E, int64_t row0, int64_t nrows,
                                               void* workspace, size_t workspace_bytes, void* stream) {
    VIPANT_REQUIRE(B >= 1 && B < (1ll << 30) && E % 64 == 0 && E >= 64 && E <= 1024, VIPANT_EBADSHAPE,
                   "sigmoid_loss: need B >= 1, E %% 64 == 0 and 64 <= E <= 1024 (B=%ld E=%ld)", (long)B, (long)E);
    VIPANT_REQUIRE(row0 >= 0 && nrows > 0 && row0 + nrows <= B, VIPANT_EBADSHAPE, "sigmoid_loss: bad row slice [%ld, %ld) of %ld",
                   (long)row0, (long)(row0 + nrows), (long)B);
    VIPANT_REQUIRE(x1 != nullptr && x2 != nullptr && logit_scale != nullptr && logit_bias != nullptr && loss != nullptr, VIPANT_EBADSHAPE,
                   "sigmoid_loss: x1, x2, logit_scale, logit_bias and loss are required");
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= vipant_sigmoid_loss_workspace_bytes(B, E, nrows), VIPANT_ENOWORKSPACE,
                   "sigmoid_loss: workspace too small (%zu bytes needed, %zu given)", vipant_sigmoid_loss_workspace_bytes(B, E, nrows),
                   workspace_bytes);
    VIPANT_REQUIRE((uintptr_t)workspace % 256 == 0, VIPANT_EALIGN, "sigmoid_loss: workspace must be 256-byte aligned");
    VIPANT_REQUIRE((uintptr_t)dx1 % 16 == 0 && (uintptr_t)dx2 % 16 == 0, VIPANT_EALIGN, "sigmoid_loss: dx1 / dx2 must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const SigWs w = sig_carve((char*)workspace, B, E, nrows);
    hipLaunchKernelGGL(sig_prep_kernel, dim3((unsigned)(E / 64), (unsigned)ceil_div(w.Bp, 64), 2), dim3(256), 0, s, x1, x2, logit_scale,
                       logit_bias, scale_max, w, (int)B, (int)E);
    VIPANT_LAUNCH_CHECK();
    // E <= 512: one chunk of E columns; above: two chunks of ceil(E / 128) * 64
    const int nct = (int)(E <= 512 ? E / 64 : ceil_div(E, 128));
    int32_t rc = VIPANT_EBADSHAPE;
    switch (nct) {
        case 1: rc = sig_launch_walk<1>(w, B, E, dx1, dx2, row0, nrows, grad_scale, s); break;
        case 2: rc = sig_launch_walk<2>(w, B, E, dx1, dx2, row0, nrows, grad_scale, s); break;
        case 3: rc = sig_launch_walk<3>(w, B, E, dx1, dx2, row0, nrows, grad_scale, s); break;
        case 4: rc = sig_launch_walk<4>(w, B, E, dx1, dx2, row0, nrows, grad_scale, s); break;
        case 5: rc = sig_launch_walk<5>(w, B, E, dx1, dx2, row0, nrows, grad_scale, s); break;
        case 6: rc = sig_launch_walk<6>(w, B, E, dx1, dx2, row0, nrows, grad_scale, s); break;
        case 7: rc = sig_launch_walk<7>(w, B, E, dx1, dx2, row0, nrows, grad_scale, s); break;
        case 8: rc = sig_launch_walk<8>(w, B, E, dx1, dx2, row0, nrows, grad_scale, s); break;
    }
    if (rc != VIPANT_OK) return rc;
    hipLaunchKernelGGL(sig_fold_kernel, dim3(1), dim3(256), 0, s, w, (int)B, grad_scale, loss, dlogit_scale, dlogit_bias);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}
