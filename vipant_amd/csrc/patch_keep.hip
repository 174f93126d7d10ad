// Patchout at the token boundary: the patch embedding over a KEPT subset of each clip's patches.
//
// Forward: an implicit GEMM with a row indirection.  A workgroup (four waves) owns 64 kept patches of ONE clip and 256 columns of the
// width; it never sees an im2col matrix.  Per 64-deep K-chunk its 256 threads read the chunk's 64 x 64 fp32 straight from the
// spectrogram -- one thread = 8 consecutive fp32 of one patch row segment (pw % 8 == 0: a group never leaves its segment), two
// 16-byte loads --, round to bf16 and store 16 bytes into LDS: rows of 128 bytes, the 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7),
// the swizzle of nt_core.h, so that the A-fragment reads of v_mfma_f32_16x16x32_bf16 (16 rows x 4 chunks per wave) touch every bank
// group once.  Two 8 KiB buffers (16 KiB of LDS): chunk kt + 1 is loaded into registers before chunk kt is contracted, and stored
// behind it; one barrier per chunk.  The w_eff fragments (wave w: columns 64 w .. 64 w + 63 of the tile) come from global memory -- the
// matrix is 0.4 - 1.5 MB and stays in L2 -- a chunk ahead, in registers.  The column tile of 256 splits into the four waves' 64, and the
// width is a multiple of 64: a ragged last column tile leaves whole waves idle (they still load A), never a partial fragment.  The
// epilogue adds the GATHERED positional row pos[1 + keep] and stores fp32; the first column tile of a row tile also writes the bf16
// rows it put into LDS to `patches` (the operand of the weight gradient), from the registers that hold the LDS image.
//
// Backward: inv[b, P] (slot of a patch in its clip's list, or -1; a binary search per entry, the lists ascend), the bf16 rounding of
// the kept token rows' gradient, and dpos / dcls without atomics: one thread owns (position, four columns) and walks the items in
// ascending order, eight loads in flight, one add after the other -- the same bits every run.
#include "common.h"

namespace {

constexpr int KEEP_BM = 64, KEEP_BN = 256, KEEP_BK = 64;
constexpr int KEEP_STAGE = KEEP_BM * KEEP_BK * 2;        // 8 KiB: one K-chunk of the kept rows in bf16

struct KeepGeom {
    int C, T, F, Dw, ph, pw, sh, sw, ncol, P, k;
};

template <bool VEC>
__global__ __launch_bounds__(256) void patch_keep_tokens_kernel(const float* __restrict__ x, const bf16_t* __restrict__ w,
                                                                const float* __restrict__ pos, const int* __restrict__ keep,
                                                                float* __restrict__ tokens, bf16_t* __restrict__ patches, KeepGeom g) {
    __shared__ __attribute__((aligned(16))) char smem[2 * KEEP_STAGE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n0 = blockIdx.x * KEEP_BN, slot0 = blockIdx.y * KEEP_BM, item = blockIdx.z;
    const int khw = g.ph * g.pw, kcols = g.C * khw, nk = kcols / KEEP_BK;
    const bool store_rows = patches != nullptr && blockIdx.x == 0;

    // ---- loader role: chunk lc of rows lr and lr + 32
    const int lc = tid & 7;
    int64_t xbase[2], prow[2];
    bool live[2], listed[2];
    uint32_t lds_at[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = (tid >> 3) + 32 * h, slot = slot0 + r;
        listed[h] = slot < g.k;
        const int p = listed[h] ? keep[(int64_t)item * g.k + slot] : -1;
        live[h] = p >= 0 && p < g.P;            // an entry outside the grid is never turned into an address
        const int tr = live[h] ? p / g.ncol : 0, fc = live[h] ? p - tr * g.ncol : 0;
        xbase[h] = ((int64_t)item * g.C * g.T + (int64_t)tr * g.sh) * g.F + (int64_t)fc * g.sw;
        prow[h] = (int64_t)item * g.k + slot;
        lds_at[h] = (uint32_t)(r * 128 + ((lc ^ ((r >> 1) & 7)) << 4));
    }
    f32x4 xa[2][2];
    auto load_x = [&](int kt) {
        const int kk = kt * KEEP_BK + lc * 8;
        const int c = kk / khw, rem = kk - c * khw, ii = rem / g.pw, jj = rem - ii * g.pw;
        const int64_t off = ((int64_t)c * g.T + ii) * g.F + jj;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            xa[h][0] = xa[h][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live[h]) {
                const float* src = x + xbase[h] + off;
                if constexpr (VEC) {
                    xa[h][0] = *(const f32x4*)src;
                    xa[h][1] = *(const f32x4*)(src + 4);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { xa[h][0][e] = src[e]; xa[h][1][e] = src[4 + e]; }
                }
            }
        }
    };
    auto store_x = [&](int stage, int kt) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) { o[e] = (bf16_t)xa[h][0][e]; o[4 + e] = (bf16_t)xa[h][1][e]; }
            *(bf16x8*)(smem + stage * KEEP_STAGE + lds_at[h]) = o;
            if (store_rows && listed[h]) *(bf16x8*)(patches + prow[h] * kcols + kt * KEEP_BK + lc * 8) = o;
        }
    };

    // ---- contraction role: wave w owns columns n0 + 64 w .. + 63 of all 64 rows
    const int frow = lane & 15, fq = lane >> 4, fs = (lane >> 1) & 7;
    const bool active = n0 + wave * 64 < g.Dw;              // (Dw % 64 == 0: a wave's 64 columns are all inside, or none is)
    uint32_t offA[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) offA[ks] = (uint32_t)(frow * 128 + (((ks * 4 + fq) ^ fs) << 4));
    const bf16_t* wb = w + (int64_t)(n0 + wave * 64 + frow) * kcols + fq * 8;
    bf16x8 bc[2][4], bn[2][4];
    auto load_b = [&](bf16x8 (&b)[2][4], int kt) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int j = 0; j < 4; ++j) b[ks][j] = *(const bf16x8*)(wb + (int64_t)j * 16 * kcols + kt * KEEP_BK + ks * 32);
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_x(0);
    if (active) load_b(bc, 0);
    store_x(0, 0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) {
            load_x(kt + 1);
            if (active) load_b(bn, kt + 1);
        }
        if (active) {
            const char* s = smem + cur * KEEP_STAGE;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 a[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = *(const bf16x8*)(s + offA[ks] + i * 2048);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bc[ks][j], a[i], acc[i][j], 0, 0, 0);
            }
        }
        // the other buffer was last read in step kt - 1, and every wave has passed that step's barrier
        if (more) store_x(cur ^ 1, kt + 1);
        __syncthreads();
        cur ^= 1;
        if (more && active) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int j = 0; j < 4; ++j) bc[ks][j] = bn[ks][j];
        }
    }
    if (!active) return;
    // ---- epilogue: acc[i][j][e] = row i * 16 + (lane & 15), column n0 + 64 wave + j * 16 + (lane >> 4) * 4 + e
    const int S1 = g.k + 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int slot = slot0 + i * 16 + frow;
        if (slot >= g.k) continue;
        const int p = keep[(int64_t)item * g.k + slot];
        if (p < 0 || p >= g.P) continue;
        float* dst = tokens + ((int64_t)item * S1 + 1 + slot) * g.Dw + n0 + wave * 64 + fq * 4;
        const float* pr = pos + (int64_t)(1 + p) * g.Dw + n0 + wave * 64 + fq * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) *(f32x4*)(dst + j * 16) = acc[i][j] + *(const f32x4*)(pr + j * 16);
    }
}

// inv[item, p] = the slot m with keep[item, m] == p, or -1: the lists ascend, so a binary search per entry (no fill-then-scatter,
// no ordering between two writers of one word)
__global__ __launch_bounds__(256) void keep_inverse_kernel(const int* __restrict__ keep, int* __restrict__ inv, int64_t b, int k, int P) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < b * P; i += (int64_t)gridDim.x * 256) {
        const int p = (int)(i % P);
        const int* row = keep + (i / P) * k;
        int lo = 0, hi = k;                     // first slot whose entry is >= p
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (row[mid] < p) lo = mid + 1; else hi = mid;
        }
        inv[i] = (lo < k && row[lo] == p) ? lo : -1;
    }
}

// dpatches[item * k + m] = bf16 (round to nearest even) of dtokens[item * (k + 1) + 1 + m]
__global__ __launch_bounds__(256) void keep_dpatches_kernel(const float* __restrict__ dtok, bf16_t* __restrict__ dpatches, int64_t b,
                                                            int k, int D) {
    const int d4 = D / 4;
    const int64_t total = b * k * d4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % d4) * 4;
        const int64_t row = i / d4, item = row / k;
        *(bf16x4*)(dpatches + row * D + c) = f32x4_to_bf16x4(*(const f32x4*)(dtok + (row + item + 1) * D + c));
    }
}

// dpos[s] = sum over the items that have a token at position s of that token's gradient row, in ascending item order; s = 0 is the
// class token (every item: also dcls); positions nobody kept come out as zeros
__global__ __launch_bounds__(256) void keep_dpos_kernel(const float* __restrict__ dtok, const int* __restrict__ inv, float* __restrict__ dcls,
                                                        float* __restrict__ dpos, int64_t b, int k, int P, int D) {
    const int d4 = D / 4, S1 = k + 1;
    const int64_t total = (int64_t)(P + 1) * d4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % d4) * 4, s = (int)(i / d4);
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t bi = 0; bi < b; bi += 8) {
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {       // eight independent loads in flight
                const int64_t item = bi + j;
                int row = -1;
                if (item < b) row = s == 0 ? 0 : inv[item * P + s - 1] + 1;        // (-1 + 1 = 0 marks "not kept" for s > 0)
                const bool has = item < b && (s == 0 || row > 0);
                v[j] = has ? *(const f32x4*)(dtok + (item * S1 + row) * D + c) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) acc += v[j];        // one after the other: ascending item order
        }
        if (s == 0) *(f32x4*)(dcls + c) = acc;
        *(f32x4*)(dpos + (int64_t)s * D + c) = acc;
    }
}

int grid_of(int64_t n, int per, int cap) {
    const int64_t g = ceil_div(n, per);
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

#define TRY(expr)                         \
    do {                                  \
        const int32_t _rc = (expr);       \
        if (_rc != VIPANT_OK) return _rc; \
    } while (0)

// the shape rules of the kept-patch embedding: everything vipant_patch_embed_ln_fwd refuses, and the list
int32_t keep_shape_check(const char* op, const int32_t* keep, int64_t b, int64_t C, int64_t T, int64_t F, int64_t Dw, int64_t ph, int64_t pw,
                         int64_t sh, int64_t sw, int64_t k) {
    VIPANT_REQUIRE(b > 0 && C > 0 && Dw > 0 && ph > 0 && pw > 0 && sh > 0 && sw > 0, VIPANT_EBADSHAPE,
                   "%s: every extent and stride must be positive (b=%ld C=%ld Dw=%ld ph=%ld pw=%ld sh=%ld sw=%ld)", op, (long)b, (long)C,
                   (long)Dw, (long)ph, (long)pw, (long)sh, (long)sw);
    VIPANT_REQUIRE(T >= ph && F >= pw && pw % 8 == 0, VIPANT_EBADSHAPE, "%s: need T>=ph, F>=pw, pw%%8==0 (T=%ld F=%ld ph=%ld pw=%ld)", op,
                   (long)T, (long)F, (long)ph, (long)pw);
    const int64_t P = ((T - ph) / sh + 1) * ((F - pw) / sw + 1);
    VIPANT_REQUIRE((C * ph * pw) % 64 == 0, VIPANT_EBADSHAPE, "%s: C * ph * pw must be a multiple of 64 (%ld)", op, (long)(C * ph * pw));
    VIPANT_REQUIRE(ln_width_ok(Dw), VIPANT_EBADSHAPE, "%s: the width must be a multiple of 64 from 192 to 1024 (Dw=%ld)", op, (long)Dw);
    VIPANT_REQUIRE(keep != nullptr, VIPANT_EBADSHAPE, "%s: no list of kept patches", op);
    VIPANT_REQUIRE(k >= 1 && k <= P, VIPANT_EBADSHAPE, "%s: need 1 <= k <= P (k=%ld P=%ld)", op, (long)k, (long)P);
    VIPANT_REQUIRE(b <= 65535 && C * T * F < (1ll << 31) && C * ph * pw < (1ll << 31) && P < (1ll << 31), VIPANT_EBADSHAPE,
                   "%s: more than 65535 clips, or a clip of 2^31 elements", op);
    return VIPANT_OK;
}

}  // namespace

extern "C" int32_t vipant_patch_keep_tokens(const float* x, const uint16_t* w_eff, const float* pos, const int32_t* keep, float* tokens,
                                            uint16_t* patches, int64_t b, int64_t C, int64_t T, int64_t F, int64_t Dw, int64_t ph,
                                            int64_t pw, int64_t sh, int64_t sw, int64_t k, void* stream) {
    TRY(keep_shape_check("patch_keep_tokens", keep, b, C, T, F, Dw, ph, pw, sh, sw, k));
    VIPANT_REQUIRE(x != nullptr && w_eff != nullptr && pos != nullptr && tokens != nullptr && (uintptr_t)w_eff % 16 == 0 &&
                       (uintptr_t)pos % 16 == 0 && (uintptr_t)tokens % 16 == 0 && (patches == nullptr || (uintptr_t)patches % 16 == 0),
                   VIPANT_EALIGN, "patch_keep_tokens: w_eff, pos, tokens and patches must be 16-byte aligned");
    const int ncol = (int)((F - pw) / sw + 1), nrow = (int)((T - ph) / sh + 1);
    const KeepGeom g{(int)C, (int)T, (int)F, (int)Dw, (int)ph, (int)pw, (int)sh, (int)sw, ncol, nrow * ncol, (int)k};
    const dim3 grid((unsigned)ceil_div(Dw, KEEP_BN), (unsigned)ceil_div(k, KEEP_BM), (unsigned)b);
    const bool vec = F % 4 == 0 && sw % 4 == 0 && (uintptr_t)x % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(patch_keep_tokens_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)w_eff, pos, keep, tokens,
                           (bf16_t*)patches, g);
    else
        hipLaunchKernelGGL(patch_keep_tokens_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, (const bf16_t*)w_eff, pos, keep, tokens,
                           (bf16_t*)patches, g);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" int32_t vipant_patch_keep_inverse(const int32_t* keep, int32_t* inv, int64_t b, int64_t k, int64_t P, void* stream) {
    VIPANT_REQUIRE(keep != nullptr && inv != nullptr && b > 0 && P > 0 && P < (1ll << 31) && k >= 1 && k <= P, VIPANT_EBADSHAPE,
                   "patch_keep_inverse: need the list, b > 0 and 1 <= k <= P (b=%ld k=%ld P=%ld)", (long)b, (long)k, (long)P);
    hipLaunchKernelGGL(keep_inverse_kernel, dim3(grid_of(b * P, 256, 4096)), dim3(256), 0, (hipStream_t)stream, keep, inv, b, (int)k, (int)P);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" int32_t vipant_assemble_tokens_keep_bwd(const float* dtokens, const int32_t* inv, uint16_t* dpatches, float* dcls, float* dpos,
                                                   int64_t b, int64_t k, int64_t P, int64_t D, void* stream) {
    VIPANT_REQUIRE(dtokens != nullptr && inv != nullptr && dpatches != nullptr && dcls != nullptr && dpos != nullptr && b > 0 && P > 0 &&
                       P < (1ll << 31) && k >= 1 && k <= P && D > 0 && D % 4 == 0,
                   VIPANT_EBADSHAPE, "assemble_tokens_keep_bwd: need every buffer, b > 0, 1 <= k <= P and D %% 4 == 0 (b=%ld k=%ld P=%ld D=%ld)",
                   (long)b, (long)k, (long)P, (long)D);
    hipLaunchKernelGGL(keep_dpatches_kernel, dim3(grid_of(b * k * D / 4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, dtokens,
                       (bf16_t*)dpatches, b, (int)k, (int)D);
    hipLaunchKernelGGL(keep_dpos_kernel, dim3(grid_of((P + 1) * D / 4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, dtokens, inv, dcls, dpos,
                       b, (int)k, (int)P, (int)D);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" int32_t vipant_patch_embed_keep_ln_fwd(const float* x, const float* conv_w, const float* cls, const float* pos, const float* gamma,
                                                  const float* beta, const int32_t* keep, uint16_t* w_eff, uint16_t* patches, float* tokens,
                                                  float* out, float* mean, float* rstd, int64_t b, int64_t C, int64_t T, int64_t F,
                                                  int64_t Dw, int64_t Cw, int64_t ph, int64_t pw, int64_t sh, int64_t sw, int64_t k,
                                                  int32_t mean_channels, void* stream) {
    // every refusal comes before the first launch: a refused call writes nothing
    VIPANT_REQUIRE(Cw > 0, VIPANT_EBADSHAPE, "patch_embed_keep_ln_fwd: the kernel has no channels (Cw=%ld)", (long)Cw);
    TRY(keep_shape_check("patch_embed_keep_ln_fwd", keep, b, C, T, F, Dw, ph, pw, sh, sw, k));
    VIPANT_REQUIRE(C == (mean_channels ? 1 : Cw), VIPANT_EBADSHAPE, "patch_embed_keep_ln_fwd: the input has %ld channels, the %s kernel takes %ld",
                   (long)C, mean_channels ? "channel-mean" : "stored", (long)(mean_channels ? 1 : Cw));
    const int64_t S1 = k + 1;
    TRY(vipant_conv_weight_prep(conv_w, w_eff, Dw, Cw, ph * pw, mean_channels, stream));
    TRY(vipant_patch_keep_tokens(x, w_eff, pos, keep, tokens, patches, b, C, T, F, Dw, ph, pw, sh, sw, k, stream));
    TRY(vipant_tokens_cls_rows(cls, pos, tokens, b, S1, Dw, stream));
    return vipant_layernorm_fwd(tokens, Dw, gamma, beta, nullptr, out, mean, rstd, b * S1, Dw, nullptr, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" size_t vipant_patch_embed_keep_ln_bwd_workspace_bytes(int64_t b, int64_t k, int64_t Dw, int64_t kcols) {
    return max_sz(vipant_gemm_tn_workspace_bytes(b * k, Dw, kcols), vipant_layernorm_bwd_workspace_bytes(b * (k + 1), Dw));
}

extern "C" int32_t vipant_patch_embed_keep_ln_bwd(const void* dout, int32_t dout_bf16, const float* tokens, const float* mean, const float* rstd,
                                                  const float* gamma, const uint16_t* patches, const int32_t* keep, int32_t* inv,
                                                  float* dtokens, uint16_t* dpatches, float* dw_eff, float* dconv, float* dcls, float* dpos,
                                                  float* dgamma, float* dbeta, int64_t b, int64_t k, int64_t P, int64_t Dw, int64_t Cw,
                                                  int64_t khw, int32_t mean_channels, void* workspace, size_t workspace_bytes, void* stream) {
    VIPANT_REQUIRE(keep != nullptr && inv != nullptr && b > 0 && P > 0 && P < (1ll << 31) && k >= 1 && k <= P && Cw > 0 && khw > 0 &&
                       ln_width_ok(Dw),
                   VIPANT_EBADSHAPE, "patch_embed_keep_ln_bwd: need the list and its inverse, b > 0, 1 <= k <= P and a width 64 H (b=%ld k=%ld P=%ld Dw=%ld)",
                   (long)b, (long)k, (long)P, (long)Dw);
    const int64_t kcols = (mean_channels ? 1 : Cw) * khw;
    VIPANT_REQUIRE(workspace_bytes >= vipant_patch_embed_keep_ln_bwd_workspace_bytes(b, k, Dw, kcols), VIPANT_ENOWORKSPACE,
                   "patch_embed_keep_ln_bwd: workspace too small");
    TRY(vipant_layernorm_bwd(dout, dout_bf16 ? 0 : VIPANT_LN_DY_F32, tokens, Dw, mean, rstd, gamma, nullptr, dtokens, Dw, nullptr, dgamma,
                             dbeta, nullptr, 0, b * (k + 1), Dw, workspace, workspace_bytes, nullptr, nullptr, stream));
    TRY(vipant_patch_keep_inverse(keep, inv, b, k, P, stream));
    // rows 0 .. P of dpos (and dcls) are overwritten, whatever they held; rows beyond P are not touched
    TRY(vipant_assemble_tokens_keep_bwd(dtokens, inv, dpatches, dcls, dpos, b, k, P, Dw, stream));
    TRY(vipant_gemm_tn(dpatches, Dw, patches, kcols, dw_eff, kcols, b * k, Dw, kcols, 0, nullptr, workspace, workspace_bytes, stream));
    if (mean_channels) return vipant_conv_weight_grad(dw_eff, dconv, Dw, Cw, khw, 0, stream);
    return VIPANT_OK;       // dconv == dw_eff viewed as [Dw, Cw, kh, kw]
}
