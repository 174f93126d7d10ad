// Similarity-weighted symmetric InfoNCE (continuously weighted contrastive learning: CWCL; SoftCLIP and ALBEF's momentum targets are the
// same family): the soft-max target of row i is spread over the batch in proportion to a weight taken from a frozen "teacher"
// modality's own pairwise similarity,
//   s = min(exp(logit_scale), scale_max);  z_ij = s <x1_i, x2_j>;  c_ij = <t_i, t_j>;
//   W_ii = 1;  W_ij = clamp((c_ij - w_floor) / (1 - w_floor), 0, 1) ^ w_power  (i != j);  n_i = sum_j W_ij  (W is symmetric);
//   loss = (1/B) sum_i [ lse_j z_ij - (1/n_i) sum_j W_ij z_ij ] + (1/B) sum_j [ lse_i z_ij - (1/n_j) sum_i W_ij z_ij ];
//   G_ij = ( exp(z_ij - rlse_i) + exp(z_ij - clse_j) - W_ij (1/n_i + 1/n_j) ) / B;  dx1 = s G x2;  dx2 = s G^T x1;
//   dlogit_scale = sum_ij G_ij z_ij  (0 where the clamp is active).
// t == NULL is W = I: vipant_infonce_fwd_bwd's loss.  This is label_nce.hip's loss with a real-valued W computed on the fly in place
// of the 0/1 P: a SECOND MFMA product per tile of the pair matrix, and still nothing B x B or nrows x B reaches HBM.
//
// gfx950 design (four launches, label_nce.hip's: prep, stats walk over the batch, fold, gradient walk over the strip) with a new walk:
//   prep   64 x 64 tiles of x1, x2 and (unless it aliases one of them) t: the bf16 split [hi | lo] of every row ([B][2K]); for x1 and
//          x2 also the transposed bf16 copy [E][Bp] (Bp = B rounded up to 64, zero beyond B); s and the clamp flag.
//   walk   workgroup = 64 query rows (wave w owns rows 16 w .. 16 w + 15 and ALL keys: nothing is merged across waves) x 64-key tiles.
//          BOTH sides of both products are streamed the way a GEMM K-loop does it: a stage holds the hi and the lo plane of 64 query
//          rows and of 64 key rows over 64 elements of K (4 x 8 KiB, 128-byte rows, XOR-swizzled 16-byte columns), wave w fetches plane
//          w with eight LDS-DMA instructions, and two stages alternate: the loads of the next slice -- the next product's or the next
//          key tile's first slice included -- are in flight under the current slice's MFMAs.  A resident query side does not fit: 64
//          rows of [hi | lo] of x and of t are 256 KiB at E = Et = 512, and as register fragments 256 VGPRs per lane.  A key row is
//          fetched B / 64 times per side (label_nce.hip: B / 16), at the price of fetching a query row as often.
//          Per key tile: Et / 64 slices of the teacher product, then W for the lane's 16 pairs (query lane & 15, keys 16 t + 4 (lane >> 4)
//          + i), then E / 64 slices of the logit product into the same accumulators.  Both products: keys as the A operand, three terms
//          hi.hi + (hi.lo + lo.hi) on v_mfma_f32_16x16x32_bf16 -- fp32 grade at every pair, because exp(z - lse) cancels against
//          W (1/n_i + 1/n_j) wherever W is large and an error in c reaches W multiplied by w_power / (1 - w_floor).
//   stats  epilogue of a tile: the lane folds its 16 logits into an online (max, sum exp, sum exp z) triple, sum W z and sum W; the four
//          lane groups of a query merge through LDS in a fixed order.  Outputs: rlse / clse [B], 1 / n [B], per workgroup the partial
//          sums of the loss and of sum G z.
//   grad   (strip rows, side, E-chunk of <= 512 columns): the transposed key slice [chunk columns][64 keys] of the tile is a third LDS
//          region (single: it is requested at the tile's first slice and read after its last), G is rounded once to bf16 and is the B
//          operand of dx^T[16 columns x 16 queries] += x_key^T . G^T straight from the registers (sigmoid_loss.hip's K-slot order).
//   fold   one workgroup adds the stats partials in a fixed order (fp64).
// LDS: 64 KiB of stages + 128 B per chunk column (<= 64 KiB) + 1.8 KiB of reduction arrays.  One workgroup of four waves per CU.
// Deterministic: no atomics; every sum has a fixed order.  exp / log in fp32.
#include "common.h"

namespace {

struct SnceWs {     // carved out of the caller's workspace; every offset 256-B aligned
    bf16_t *xs1, *xs2;      // [B][2E]: hi | lo
    bf16_t* ts;             // [B][2Et]: hi | lo of the teacher rows (the call points it at xs1 / xs2 when t aliases x1 / x2)
    bf16_t *xt1, *xt2;      // [E][Bp]: bf16(x)^T, columns B .. Bp zero
    float *rlse, *clse;     // [Bp]: log-sum-exp of the rows / columns of z (B live)
    float* rn;              // [Bp]: 1 / n (B live)
    float* scal;            // s, clamp flag
    float* part;            // [nblk][2 sides][2]: loss and sum G z terms of a block of 64 queries
    int Bp, nblk;
    size_t total;
};

struct SnceArgs {
    int B, E, Et;           // Et == 0: no teacher, W = I
    float wfloor, winv, wpower;     // winv = 1 / (1 - w_floor)
    float *dx1, *dx2;
    int row0, nrows;
    float gscale;
};

size_t snce_align256(size_t x) { return (x + 255) & ~(size_t)255; }

SnceWs snce_carve(char* base, int64_t B, int64_t E, int64_t Et) {
    SnceWs w;
    w.Bp = (int)((B + 63) / 64 * 64);
    w.nblk = (int)ceil_div(B, 64);
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += snce_align256(bytes); return p; };
    w.xs1 = (bf16_t*)take((size_t)B * 2 * E * 2);
    w.xs2 = (bf16_t*)take((size_t)B * 2 * E * 2);
    w.ts = (bf16_t*)take((size_t)B * 2 * Et * 2);
    w.xt1 = (bf16_t*)take((size_t)E * w.Bp * 2);
    w.xt2 = (bf16_t*)take((size_t)E * w.Bp * 2);
    w.rlse = (float*)take((size_t)w.Bp * 4);
    w.clse = (float*)take((size_t)w.Bp * 4);
    w.rn = (float*)take((size_t)w.Bp * 4);
    w.scal = (float*)take(256);
    w.part = (float*)take((size_t)w.nblk * 4 * 4);
    w.total = off;
    return w;
}

// grid (max(E, Et) / 64, Bp / 64, 2 or 3 operands: x1, x2, a separate t)
__global__ __launch_bounds__(256) void snce_prep_kernel(const float* __restrict__ x1, const float* __restrict__ x2, const float* __restrict__ t,
                                                        const float* __restrict__ logit_scale, float scale_max, SnceWs w, int B, int E,
                                                        int Et) {
    __shared__ bf16_t tile[64][66];
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
        const float raw = expf(logit_scale[0]);
        const bool clamped = scale_max > 0.f && raw > scale_max;
        w.scal[0] = clamped ? scale_max : raw;
        w.scal[1] = clamped ? 1.f : 0.f;
    }
    const int op = blockIdx.z, K = op == 2 ? Et : E;
    const int tr = blockIdx.y * 64, tc = blockIdx.x * 64;
    if (tc >= K) return;
    const float* src = op == 0 ? x1 : (op == 1 ? x2 : t);
    bf16_t* xs = op == 0 ? w.xs1 : (op == 1 ? w.xs2 : w.ts);
    bf16_t* xt = op == 0 ? w.xt1 : w.xt2;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) {
        const int gr = tr + r, gc = tc + tx;
        bf16_t hi = (bf16_t)0.0f;
        if (gr < B) {
            const float v = src[(int64_t)gr * K + gc];
            hi = (bf16_t)v;
            xs[(int64_t)gr * 2 * K + gc] = hi;
            xs[(int64_t)gr * 2 * K + K + gc] = (bf16_t)(v - (float)hi);
        }
        tile[r][tx] = hi;
    }
    if (op == 2) return;            // the teacher only enters K-contiguous products
    __syncthreads();
    for (int c = ty; c < 64; c += 4) xt[(int64_t)(tc + c) * w.Bp + tr + tx] = tile[tx][c];
}

constexpr int SNCE_PLANE = 8192, SNCE_STAGE = 4 * SNCE_PLANE;      // [64 rows][64 bf16]; query hi, query lo, key hi, key lo
constexpr int SNCE_XT = 2 * SNCE_STAGE;                             // the gradient walk's transposed key slice

__device__ __forceinline__ uint32_t snce_lim(int64_t bytes) { return (uint32_t)(bytes > 0xFFFFFFFFll ? 0xFFFFFFFFll : bytes); }

// One walk for both passes.  GRAD == false: grid (ceil(B / 64), 2 sides), the statistics; GRAD == true: grid (ceil(nrows / 64), 2 sides,
// E-chunks of 64 NCT columns), the gradients of the strip.  Dynamic LDS: two stages (+ 128 B per chunk column).
template <bool GRAD, int NCT>
__global__ __launch_bounds__(256) void snce_walk_kernel(SnceWs w, SnceArgs a) {
    extern __shared__ __attribute__((aligned(16))) char snce_smem[];
    __shared__ float red[4][4][5][16];          // [wave][lane group][max, sum exp, sum exp z, sum W z, sum W][query]
    __shared__ float term[2][64];
    constexpr int NT = 4 * NCT;                 // 16-column tiles of the chunk
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), r = lane & 15, g = lane >> 4;
    const int blk = blockIdx.x, side = blockIdx.y, col0 = GRAD ? blockIdx.z * (64 * NCT) : 0;
    const int B = a.B, E = a.E, Et = a.Et;
    float* dx = side == 0 ? a.dx1 : a.dx2;
    if (GRAD && dx == nullptr) return;
    const bf16_t* xq = side == 0 ? w.xs1 : w.xs2;       // queries
    const bf16_t* xk = side == 0 ? w.xs2 : w.xs1;       // keys, K-contiguous (the logit product)
    const bf16_t* xt = side == 0 ? w.xt2 : w.xt1;       // keys, transposed (the gradient product)
    const int q0 = (GRAD ? a.row0 : 0) + 64 * blk;      // first query row of the workgroup (a row of the batch)
    const int ml = 64 * blk + 16 * wave + r, m = (GRAD ? a.row0 : 0) + ml;      // this lane's query: row of the grid, row of the batch
    const bool qlive = GRAD ? ml < a.nrows : m < B;
    const int mc = m < B ? m : B - 1;
    const float s = w.scal[0], inv_b = 1.0f / (float)B;
    const bool pow1 = a.wpower == 1.0f;
    const int nkc = Et / 64, nkz = E / 64, S = nkc + nkz, ntiles = w.Bp / 64;

    // wave `wave` fetches plane `wave` of a stage: (query | key) x (hi | lo).  Rows past the batch lie beyond the descriptor: zeros.
    const int frow = lane >> 3, fslot = lane & 7;
    auto issue = [&](int stage, int tile, int step) {
        const bool isz = step >= nkc;
        const int K = isz ? E : Et, kt = isz ? step - nkc : step;
        const bf16_t* arr = isz ? (wave < 2 ? xq : xk) : w.ts;
        const auto rs = make_rsrc(arr, snce_lim((int64_t)B * K * 4));
        const uint32_t row0 = (uint32_t)(wave < 2 ? q0 : 64 * tile), rowb = (uint32_t)K * 4;
        const uint32_t soff = (uint32_t)(((wave & 1) * K + kt * 64) * 2);
        char* dst = snce_smem + stage * SNCE_STAGE + wave * SNCE_PLANE;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int rr = i * 8 + frow;
            lds_dma16(rs, dst + i * 1024, (row0 + rr) * rowb + (uint32_t)((fslot ^ ((rr >> 1) & 7)) << 4), soff);
        }
    };
    // the transposed key slice [64 NCT columns][64 keys] of a tile: 128-byte rows, 16-byte column c of row j at slot c ^ (j & 7);
    // columns of a ragged chunk past E lie beyond the descriptor
    auto issue_xt = [&](int tile) {
        const auto rs = make_rsrc(xt + (int64_t)col0 * w.Bp, snce_lim((int64_t)(E - col0) * w.Bp * 2));
        for (int j = wave; j < 8 * NCT; j += 4)
            lds_dma16(rs, snce_smem + SNCE_XT + j * 1024, (uint32_t)(8 * j + frow) * (uint32_t)(w.Bp * 2) + (uint32_t)((fslot ^ frow) << 4),
                      (uint32_t)(tile * 128));
    };

    const float lq = (side == 0 ? w.rlse : w.clse)[GRAD ? mc : 0], rq = GRAD ? w.rn[mc] : 0.f;   // (the stats walk produces them)
    const float* lse_k = side == 0 ? w.clse : w.rlse;
    f32x4 acc[GRAD ? NT : 1];
#pragma unroll
    for (int ct = 0; ct < (GRAD ? NT : 1); ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mx = -INFINITY, se = 0.f, sw = 0.f, pz = 0.f, pn = 0.f;

    const uint32_t fs = (uint32_t)((r >> 1) & 7);
    const char* qfrag = snce_smem + (16 * wave + r) * 128;
    const char* kfrag = snce_smem + 2 * SNCE_PLANE + r * 128;

    issue(0, 0, 0);
    __syncthreads();
    int cur = 0;
    for (int tile = 0; tile < ntiles; ++tile) {
        const int k0 = 64 * tile;
        f32x4 ah[4], ax[4];         // hi.hi and (hi.lo + lo.hi) of the four 16-key tiles: eight independent MFMA chains
        float wv[16];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            ah[t] = f32x4{0.f, 0.f, 0.f, 0.f}; ax[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) wv[4 * t + i] = k0 + 16 * t + 4 * g + i == m ? 1.f : 0.f;
        }
        for (int step = 0; step < S; ++step) {
            const int nstep = step + 1 == S ? 0 : step + 1, ntile = step + 1 == S ? tile + 1 : tile;
            if (ntile < ntiles) issue(cur ^ 1, ntile, nstep);
            if (GRAD && step == 0) issue_xt(tile);
            const int so = cur * SNCE_STAGE;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const uint32_t cb = (((uint32_t)(ks * 4 + g)) ^ fs) << 4;
                const bf16x8 qh = *(const bf16x8*)(qfrag + so + cb), ql = *(const bf16x8*)(qfrag + so + SNCE_PLANE + cb);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const bf16x8 kh = *(const bf16x8*)(kfrag + so + t * 2048 + cb), kl = *(const bf16x8*)(kfrag + so + SNCE_PLANE + t * 2048 + cb);
                    ah[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, qh, ah[t], 0, 0, 0);
                    ax[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kh, ql, ax[t], 0, 0, 0);
                    ax[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kl, qh, ax[t], 0, 0, 0);
                }
            }
            if (step == nkc - 1) {          // the teacher product of the tile is complete: c -> W
#pragma unroll
                for (int t = 0; t < 4; ++t) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float c = ah[t][i] + ax[t][i];
                        const float u = fminf(fmaxf((c - a.wfloor) * a.winv, 0.f), 1.f);
                        const float p = pow1 ? u : (u > 0.f ? exp2f(a.wpower * log2f(u)) : 0.f);
                        if (k0 + 16 * t + 4 * g + i != m) wv[4 * t + i] = p;
                    }
                    ah[t] = f32x4{0.f, 0.f, 0.f, 0.f}; ax[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            if (step == S - 1) {            // the logits of the tile are complete
                if (!GRAD) {
                    float z[16], mx16 = -INFINITY;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const bool live = k0 + 16 * t + 4 * g + i < B;
                            const float zz = live ? s * (ah[t][i] + ax[t][i]) : -INFINITY;
                            z[4 * t + i] = zz;
                            mx16 = fmaxf(mx16, zz);
                            if (live) { pz = __builtin_fmaf(wv[4 * t + i], zz, pz); pn += wv[4 * t + i]; }
                        }
                    if (mx16 > -INFINITY) {         // at least one live key: the online soft-max step
                        const float nm = fmaxf(mx, mx16), f = expf(mx - nm);       // mx == -inf: f = 0
                        se *= f; sw *= f;
#pragma unroll
                        for (int j = 0; j < 16; ++j)
                            if (z[j] > -INFINITY) {
                                const float e = expf(z[j] - nm);
                                se += e;
                                sw = __builtin_fmaf(e, z[j], sw);
                            }
                        mx = nm;
                    }
                } else {
                    if (S == 1) __syncthreads();    // (one slice per tile: the transposed slice was requested in this very step)
                    const char* xrow = snce_smem + SNCE_XT + r * 128 + (g & 1) * 8;
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        // gradient coefficients: lane = query r, keys k0 + 32 kk + 16 tt + 4 g + i in K-slot 4 tt + i
                        bf16x8 bd;
#pragma unroll
                        for (int tt = 0; tt < 2; ++tt) {
                            const int t = 2 * kk + tt, n0 = k0 + 16 * t + 4 * g;
                            const f32x4 lk = *(const f32x4*)(lse_k + n0), rk = *(const f32x4*)(w.rn + n0);
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const float z = s * (ah[t][i] + ax[t][i]);
                                float gv = 0.f;
                                if (qlive && n0 + i < B) gv = (expf(z - lq) + expf(z - lk[i]) - wv[4 * t + i] * (rq + rk[i])) * inv_b;
                                bd[4 * tt + i] = (bf16_t)gv;
                            }
                        }
                        // dx^T[column tile x queries] += x_key^T[columns x these 32 keys] . G^T, the keys in the order the lanes hold G
                        const uint32_t c0 = (((uint32_t)(4 * kk + (g >> 1))) ^ (uint32_t)(r & 7)) << 4;
                        const uint32_t c1 = (((uint32_t)(4 * kk + 2 + (g >> 1))) ^ (uint32_t)(r & 7)) << 4;
#pragma unroll
                        for (int ct = 0; ct < NT; ++ct) {
                            if (col0 + 16 * ct < E) {
                                const u32x2 a0 = *(const u32x2*)(xrow + ct * 2048 + c0), a1 = *(const u32x2*)(xrow + ct * 2048 + c1);
                                const u32x4 av = u32x4{a0[0], a0[1], a1[0], a1[1]};
                                acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), bd, acc[ct], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            cur ^= 1;
        }
    }

    if (GRAD) {
        if (qlive) {                // lane: query r, columns col0 + 16 ct + 4 g .. + 3
            const float k = s * a.gscale;
            float* orow = dx + (int64_t)ml * E + col0 + 4 * g;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
                if (col0 + 16 * ct < E) *(f32x4*)(orow + 16 * ct) = acc[ct] * k;
        }
        return;
    }
    red[wave][g][0][r] = mx; red[wave][g][1][r] = se; red[wave][g][2][r] = sw; red[wave][g][3][r] = pz; red[wave][g][4][r] = pn;
    __syncthreads();
    if (g == 0) {                   // query r of this wave: its four lane groups, in order
        float fm = -INFINITY;
        for (int q = 0; q < 4; ++q) fm = fmaxf(fm, red[wave][q][0][r]);
        float fe = 0.f, fw = 0.f, fp = 0.f, fn = 0.f;
        for (int q = 0; q < 4; ++q) {
            const float pm = red[wave][q][0][r];
            fp += red[wave][q][3][r];
            fn += red[wave][q][4][r];
            if (pm == -INFINITY) continue;
            const float f = expf(pm - fm);
            fe = __builtin_fmaf(red[wave][q][1][r], f, fe);
            fw = __builtin_fmaf(red[wave][q][2][r], f, fw);
        }
        float tl = 0.f, tg = 0.f;
        if (qlive) {
            const float lse = fm + logf(fe), pos = fp / fn;     // n >= 1: the query's own pair
            (side == 0 ? w.rlse : w.clse)[m] = lse;
            if (side == 0) w.rn[m] = 1.0f / fn;
            tl = lse - pos;
            tg = fw / fe - pos;
        }
        term[0][16 * wave + r] = tl; term[1][16 * wave + r] = tg;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        float t = 0.f;
        for (int q = 0; q < 64; ++q) t += term[threadIdx.x][q];
        w.part[(2 * blk + side) * 2 + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(256) void snce_fold_kernel(SnceWs w, int B, float gscale, float* __restrict__ loss, float* __restrict__ dls) {
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

bool snce_width_ok(int64_t E) { return E % 64 == 0 && E >= 64 && E <= 1024; }
// B: the descriptors of the walk address a whole operand ([B][2K] bf16, [512 columns][Bp] bf16) with 32-bit byte offsets
bool snce_shape_ok(int64_t B, int64_t E, int64_t Et) { return B >= 1 && B <= (1ll << 19) && snce_width_ok(E) && (Et == 0 || snce_width_ok(Et)); }

// launch == false: only raises the kernel's dynamic-LDS limit on this device (done before the call's first launch, so that a failure
// there leaves nothing written); launch == true: the walk
template <bool GRAD, int NCT>
int32_t snce_walk(bool launch, const SnceWs& w, const SnceArgs& a, hipStream_t s) {
    const int lds = 2 * SNCE_STAGE + (GRAD ? NCT * 64 * 128 : 0);
    if (!launch) {
        static DeviceMax most;
        if (raise_on_device(most, lds)) {
            VIPANT_HIP_TRY(hipFuncSetAttribute((const void*)snce_walk_kernel<GRAD, NCT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            raised_on_device(most, lds);
        }
        return VIPANT_OK;
    }
    const dim3 grid = GRAD ? dim3((unsigned)ceil_div(a.nrows, 64), 2, (unsigned)ceil_div(a.E, 64 * NCT)) : dim3((unsigned)w.nblk, 2);
    hipLaunchKernelGGL((snce_walk_kernel<GRAD, NCT>), grid, dim3(256), lds, s, w, a);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

int32_t snce_grad_any(bool launch, const SnceWs& w, const SnceArgs& a, hipStream_t s) {
    // E <= 512: one chunk of E columns; above: two chunks of ceil(E / 128) * 64
    switch ((int)(a.E <= 512 ? a.E / 64 : ceil_div(a.E, 128))) {
        case 1: return snce_walk<true, 1>(launch, w, a, s);
        case 2: return snce_walk<true, 2>(launch, w, a, s);
        case 3: return snce_walk<true, 3>(launch, w, a, s);
        case 4: return snce_walk<true, 4>(launch, w, a, s);
        case 5: return snce_walk<true, 5>(launch, w, a, s);
        case 6: return snce_walk<true, 6>(launch, w, a, s);
        case 7: return snce_walk<true, 7>(launch, w, a, s);
        case 8: return snce_walk<true, 8>(launch, w, a, s);
    }
    return VIPANT_EBADSHAPE;
}

}  // namespace

extern "C" size_t vipant_soft_nce_workspace_bytes(int64_t B, int64_t E, int64_t Et, int64_t nrows) {
    return snce_shape_ok(B, E, Et) && nrows >= 0 && nrows <= B ? snce_carve(nullptr, B, E, Et).total : 0;
}

extern "C" int32_t vipant_soft_nce_fwd_bwd(const float* x1, const float* x2, const float* t, int64_t Et, float w_floor, float w_power,
                                           const float* logit_scale, float scale_max, float* loss, float* dx1, float* dx2,
                                           float* dlogit_scale, float grad_scale, int64_t B, int64_t E, int64_t row0, int64_t nrows,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    if (t == nullptr) Et = 0;
    VIPANT_REQUIRE(snce_shape_ok(B, E, Et) && (t == nullptr || Et > 0), VIPANT_EBADSHAPE,
                   "soft_nce: need 1 <= B <= 2^19, E %% 64 == 0 and 64 <= E <= 1024, the same range for Et (B=%ld E=%ld Et=%ld)", (long)B,
                   (long)E, (long)Et);
    VIPANT_REQUIRE(w_floor >= -1.f && w_floor < 1.f && w_power > 0.f, VIPANT_EBADSHAPE,
                   "soft_nce: need -1 <= w_floor < 1 and w_power > 0 (w_floor=%g w_power=%g)", (double)w_floor, (double)w_power);
    VIPANT_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= B, VIPANT_EBADSHAPE, "soft_nce: bad row slice [%ld, %ld) of %ld", (long)row0,
                   (long)(row0 + nrows), (long)B);
    VIPANT_REQUIRE(x1 != nullptr && x2 != nullptr && logit_scale != nullptr && loss != nullptr, VIPANT_EBADSHAPE,
                   "soft_nce: x1, x2, logit_scale and loss are required");
    const size_t need = vipant_soft_nce_workspace_bytes(B, E, Et, nrows);
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= need, VIPANT_ENOWORKSPACE,
                   "soft_nce: workspace too small (%zu bytes needed, %zu given)", need, workspace_bytes);
    VIPANT_REQUIRE((uintptr_t)workspace % 256 == 0, VIPANT_EALIGN, "soft_nce: workspace must be 256-byte aligned");
    VIPANT_REQUIRE((uintptr_t)dx1 % 16 == 0 && (uintptr_t)dx2 % 16 == 0, VIPANT_EALIGN, "soft_nce: dx1 / dx2 must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    SnceWs w = snce_carve((char*)workspace, B, E, Et);
    const bool alias = t != nullptr && Et == E && (t == x1 || t == x2);     // the split of x1 / x2 serves the teacher product as well
    if (alias) w.ts = t == x1 ? w.xs1 : w.xs2;
    const SnceArgs a{(int)B, (int)E, (int)Et, w_floor, 1.0f / (1.0f - w_floor), w_power, dx1, dx2, (int)row0, (int)nrows, grad_scale};
    const bool grads = (dx1 != nullptr || dx2 != nullptr) && nrows > 0;
    int32_t rc = snce_walk<false, 1>(false, w, a, s);      // both walks' LDS limits before the first launch: a failure leaves nothing written
    if (rc == VIPANT_OK && grads) rc = snce_grad_any(false, w, a, s);
    if (rc != VIPANT_OK) return rc;
    const int64_t kmax = Et > E ? Et : E;
    hipLaunchKernelGGL(snce_prep_kernel, dim3((unsigned)(kmax / 64), (unsigned)(w.Bp / 64), t != nullptr && !alias ? 3 : 2), dim3(256), 0, s, x1,
                       x2, t, logit_scale, scale_max, w, (int)B, (int)E, (int)Et);
    VIPANT_LAUNCH_CHECK();
    rc = snce_walk<false, 1>(true, w, a, s);
    if (rc != VIPANT_OK) return rc;
    hipLaunchKernelGGL(snce_fold_kernel, dim3(1), dim3(256), 0, s, w, (int)B, grad_scale, loss, dlogit_scale);
    VIPANT_LAUNCH_CHECK();
    return grads ? snce_grad_any(true, w, a, s) : VIPANT_OK;
}
