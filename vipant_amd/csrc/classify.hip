// Classification loss heads: soft-max cross entropy (ClassificationHead, cvap/module/decoder/loss_head.py:416-418) and binary
// cross entropy with logits (BCELossHead, cvap/module/decoder/loss_more.py:140-142) on the UNSCALED fp32 logits z of the head's
// last Linear.  One launch gives the loss, the bf16 gradient dz (the operand of the two backward contractions), the gradient of
// the log temperature and the arg-max / sigmoid the eval path caches; no B x C probability matrix is stored.
//
// Layout: one row per wave, lane l holds columns l, l + 64, ... (a wave reads 256 contiguous bytes per step).  The soft-max
// needs three passes over a row (maximum, sum, gradient): up to 16 x 64 columns stay in registers, wider rows are read again
// from memory (L2-resident: a row is a few KB).  The binary kernel needs one pass and streams it.  Row reductions are xor
// butterflies over the 64 lanes; the sums over rows are two-level and fixed-order: the four waves of a workgroup add their rows
// through LDS in wave order into part[workgroup], one workgroup then sums the partials in index order in fp64.  No float
// atomics: two runs are bit-identical.
//
// vipant_multihot_mix forms the tagging targets those heads score from ragged class-id lists (and mixup's soft targets from a
// clip's list and its partner's): one launch, every element written once by the thread that owns it.
#include "common.h"

#define CLS_WAVES 4     // rows per workgroup
#define CLS_KMAX 16     // register-resident rows: C <= 64 * CLS_KMAX

static inline int64_t cls_groups(int64_t nrows) { return ceil_div(nrows > 0 ? nrows : 1, CLS_WAVES); }

// K > 0: the row's K x 64 columns are loaded once into v[]; K == 0: every pass reads memory
template <int K>
struct ClsRow {
    float v[K > 0 ? K : 1];
    const float* p;
    int C;
    __device__ __forceinline__ void load(const float* row, int c, int lane) {
        p = row;
        C = c;
        if constexpr (K > 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int j = k * 64 + lane;
                v[k] = j < C ? row[j] : 0.f;
            }
        }
    }
    __device__ __forceinline__ int steps() const { return K > 0 ? K : (C + 63) >> 6; }
    __device__ __forceinline__ float at(int k, int j) const {      // j = k * 64 + lane < C
        if constexpr (K > 0) return v[k];
        return p[j];
    }
};

// the workgroup's CLS_WAVES per-row values, added in wave order by thread 0 into part[2 * group + {0, 1}]
__device__ __forceinline__ void cls_group_partial(float a, float b, float* __restrict__ part) {
    __shared__ float sh[2][CLS_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        sh[0][w] = a;
        sh[1][w] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float sa = sh[0][0], sb = sh[1][0];
#pragma unroll
        for (int i = 1; i < CLS_WAVES; ++i) {
            sa += sh[0][i];
            sb += sh[1][i];
        }
        part[2 * (int64_t)blockIdx.x] = sa;
        part[2 * (int64_t)blockIdx.x + 1] = sb;
    }
}

// soft-max cross entropy of x = s * z, s = exp(logit_scale).  Per row: m = max x, lse = m + log sum exp(x - m),
// loss_i = lse - x_y, r_i = d loss_i / d logit_scale = sum_j p_j (x_j - m) - (x_y - m) (p sums to 1, so the shift by m is exact
// and keeps the terms small), dz_j = g (p_j - [j == y]) with g = grad_scale * s / B.  A label outside [0, C) is clamped into the
// range (the host cannot see a device tensor's values; the kernel never indexes out of bounds).
template <int K>
__global__ __launch_bounds__(256) void softmax_ce_rows(const float* __restrict__ z, int64_t ldz, const int64_t* __restrict__ labels,
                                                       const float* __restrict__ logit_scale, bf16_t* __restrict__ dz, int64_t ldd,
                                                       int* __restrict__ pred, int row0, int nrows, float grad_scale, float inv_b,
                                                       int C, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int local = blockIdx.x * CLS_WAVES + w;
    float loss = 0.f, dls = 0.f;
    if (local < nrows) {
        const int row = row0 + local;
        const float s = expf(logit_scale[0]);
        ClsRow<K> r;
        r.load(z + (int64_t)row * ldz, C, lane);
        const int n = K > 0 ? K : r.steps();
        // row maximum of z and its first column (torch.argmax: the lowest index among exact ties)
        float best = -INFINITY;
        int arg = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < n; ++k) {
            const int j = k * 64 + lane;
            if (j < C) {
                const float t = r.at(k, j);
                if (t > best || arg == 0x7fffffff) {
                    best = t;
                    arg = j;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(arg, o, 64);
            if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) {
                best = ob;
                arg = oa;
            }
        }
        // with d_j = x_j - x_arg <= 0: sum exp(d) = 1 + rest, rest over the columns other than arg.  Keeping the 1 apart makes
        // a confident row exact: lse = log1p(rest) and 1 - p_arg = rest / (1 + rest) carry no cancellation.
        const float m = s * best;
        float rest = 0.f;
#pragma unroll
        for (int k = 0; k < n; ++k) {
            const int j = k * 64 + lane;
            if (j < C && j != arg) rest += expf(s * r.at(k, j) - m);
        }
        rest = wave_sum(rest);
        const float inv = 1.f / (1.f + rest);
        const float lse = log1pf(rest);                      // log sum exp(x - m)
        int64_t y = labels[row];
        y = y < 0 ? 0 : (y >= C ? C - 1 : y);
        const float dy = (int)y == arg ? 0.f : s * z[(int64_t)row * ldz + y] - m;      // x_y - m
        const float g = grad_scale * s * inv_b;
        float px = 0.f;
        bf16_t* drow = dz != nullptr ? dz + (int64_t)row * ldd : nullptr;
#pragma unroll
        for (int k = 0; k < n; ++k) {
            const int j = k * 64 + lane;
            if (j < C) {
                const float d = j == arg ? 0.f : s * r.at(k, j) - m;
                const float p = expf(d) * inv;
                px = __builtin_fmaf(p, d, px);
                const float q = j != (int)y ? p : (j == arg ? -rest * inv : p - 1.f);      // p_j - [j == y]
                if (drow != nullptr) drow[j] = f32_to_bf16(g * q);
            }
        }
        if (drow != nullptr)
            for (int j = C + lane; j < ldd; j += 64) drow[j] = f32_to_bf16(0.f);      // pad columns of the contractions' K
        px = wave_sum(px);
        loss = lse - dy;
        dls = px - dy;
        if (pred != nullptr && lane == 0) pred[row] = arg;
    }
    cls_group_partial(loss, dls, part);
}

// binary cross entropy with logits of x = s * z against t in {0, 1}: max(x, 0) - x t + log1p(exp(-|x|)), mean over B * C;
// dz = g (sigmoid(x) - t), g = grad_scale * s / (B C); r = d / d logit_scale = sum (sigmoid(x) - t) x.
// TG = uint8_t: binary targets (non-zero = 1).  TG = float: soft targets (mixup's lam y + (1 - lam) y'), not clamped; an element
// whose target is exactly 0 or 1 takes the binary arithmetic, so float {0, 1} targets give the uint8 kernel's bits.
template <typename TG>
__global__ __launch_bounds__(256) void bce_logits_rows(const float* __restrict__ z, int64_t ldz, const TG* __restrict__ tg,
                                                       int64_t ldt, const float* __restrict__ logit_scale, bf16_t* __restrict__ dz,
                                                       int64_t ldd, float* __restrict__ prob, int64_t ldp, int row0, int nrows,
                                                       float grad_scale, float inv_bc, int C, float* __restrict__ part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int local = blockIdx.x * CLS_WAVES + w;
    float loss = 0.f, dls = 0.f;
    if (local < nrows) {
        const int row = row0 + local;
        const float s = logit_scale != nullptr ? expf(logit_scale[0]) : 1.f;
        const float g = grad_scale * s * inv_bc;
        const float* zr = z + (int64_t)row * ldz;
        const TG* tr = tg + (int64_t)row * ldt;
        bf16_t* drow = dz != nullptr ? dz + (int64_t)row * ldd : nullptr;
        float* prow = prob != nullptr ? prob + (int64_t)row * ldp : nullptr;
        for (int j = lane; j < C; j += 64) {
            const float x = s * zr[j];
            float t;
            if constexpr (sizeof(TG) == 1) t = tr[j] != 0 ? 1.f : 0.f;
            else t = tr[j];
            const float e = expf(-fabsf(x));
            const float sg = (x >= 0.f ? 1.f : e) / (1.f + e);
            float q;
            if constexpr (sizeof(TG) == 1) q = t != 0.f ? -((x >= 0.f ? e : 1.f) / (1.f + e)) : sg;      // sigmoid(x) - t without cancellation
            else q = t == 1.f ? -((x >= 0.f ? e : 1.f) / (1.f + e)) : (t == 0.f ? sg : sg - t);
            loss += fmaxf(x, 0.f) - x * t + log1pf(e);
            dls = __builtin_fmaf(q, x, dls);
            if (drow != nullptr) drow[j] = f32_to_bf16(g * q);
            if (prow != nullptr) prow[j] = sg;
        }
        if (drow != nullptr)
            for (int j = C + lane; j < ldd; j += 64) drow[j] = f32_to_bf16(0.f);
        loss = wave_sum(loss);
        dls = wave_sum(dls);
    }
    cls_group_partial(loss, dls, part);
}

// level 2: one workgroup sums the per-group partials in index order (fp64): loss = sum * inv, dscale = grad_scale * sum * inv
__global__ __launch_bounds__(256) void cls_finish(const float* __restrict__ part, int64_t ngroups, double inv, float grad_scale,
                                                  float* __restrict__ loss, float* __restrict__ dscale) {
    __shared__ double red[2][256];
    double a = 0.0, b = 0.0;
    for (int64_t t = threadIdx.x; t < ngroups; t += 256) {
        a += (double)part[2 * t];
        b += (double)part[2 * t + 1];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(red[0][0] * inv);
        if (dscale != nullptr) dscale[0] = (float)((double)grad_scale * red[1][0] * inv);
    }
}

// ---- tagging targets from ragged class-id lists --------------------------------------------------------------------------
// One workgroup row per output row (blockIdx.x), 256 classes per workgroup and pass; every thread owns its elements y[i, c] and
// decides them by walking the clip's list and its partner's (a handful of ids each, the same addresses for the whole wave), so
// each element is written once whatever the lists hold: duplicates give 1, ids outside [0, C) match no c.  The products and the
// sum are rounded one by one (__fmul_rn / __fadd_rn: no contraction to FMA) -- the bits of `lam * y + (1 - lam) * y[p]` in torch.
__global__ __launch_bounds__(256) void multihot_mix_kernel(const int32_t* __restrict__ ids, int total, const int32_t* __restrict__ offsets,
                                                           const int32_t* __restrict__ mix_index, const float* __restrict__ mix_lambda,
                                                           float* __restrict__ y, int nsrc, int C) {
    const int row = blockIdx.x;
    auto bounds = [&](int r, int& lo, int& hi) {                  // clamped: nothing outside ids[0 : total] is read
        lo = offsets[r]; hi = offsets[r + 1];
        lo = lo < 0 ? 0 : (lo > total ? total : lo);
        hi = hi < lo ? lo : (hi > total ? total : hi);
    };
    int lo, hi, plo = 0, phi = 0;
    bounds(row, lo, hi);
    int p = -1;
    float lam = 1.f, oml = 0.f;
    if (mix_index != nullptr) {
        p = mix_index[row];
        p = p < 0 ? -1 : (p >= nsrc ? nsrc - 1 : p);
        if (p >= 0) {
            bounds(p, plo, phi);
            lam = mix_lambda[row];
            oml = __fsub_rn(1.0f, lam);
        }
    }
    for (int c = blockIdx.y * 256 + threadIdx.x; c < C; c += gridDim.y * 256) {
        float own = 0.f, par = 0.f;
        for (int k = lo; k < hi; ++k) own = ids[k] == c ? 1.f : own;
        for (int k = plo; k < phi; ++k) par = ids[k] == c ? 1.f : par;
        y[(int64_t)row * C + c] = p >= 0 ? __fadd_rn(__fmul_rn(lam, own), __fmul_rn(oml, par)) : own;
    }
}

// ---- host entry points ------------------------------------------------------------------------------------------------
extern "C" int32_t vipant_multihot_mix(const int32_t* ids, int64_t total, const int32_t* offsets, const int32_t* mix_index,
                                       const float* mix_lambda, float* y, int64_t nsrc, int64_t b, int64_t C, void* stream) {
    VIPANT_REQUIRE(ids != nullptr && offsets != nullptr && y != nullptr, VIPANT_EBADSHAPE, "multihot_mix: ids, offsets and y are required");
    VIPANT_REQUIRE(b > 0 && nsrc >= b && C > 0 && total >= 0 && nsrc < (1ll << 31) - 1 && C < (1ll << 30) && total < (1ll << 31),
                   VIPANT_EBADSHAPE, "multihot_mix: bad shape b=%ld nsrc=%ld C=%ld total=%ld", (long)b, (long)nsrc, (long)C, (long)total);
    VIPANT_REQUIRE((mix_index == nullptr) == (mix_lambda == nullptr), VIPANT_EBADSHAPE, "multihot_mix: mix_index and mix_lambda go together");
    const int64_t chunks = ceil_div(C, 256);
    hipLaunchKernelGGL(multihot_mix_kernel, dim3((unsigned)b, (unsigned)(chunks < 1024 ? chunks : 1024)), dim3(256), 0, (hipStream_t)stream,
                       ids, (int)total, offsets, mix_index, mix_lambda, y, (int)nsrc, (int)C);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" size_t vipant_softmax_ce_workspace_bytes(int64_t nrows) { return (size_t)(cls_groups(nrows) * 2 * sizeof(float)); }
extern "C" size_t vipant_bce_logits_workspace_bytes(int64_t nrows) { return (size_t)(cls_groups(nrows) * 2 * sizeof(float)); }

static int32_t cls_check(const char* who, int64_t ldz, int64_t ldd, bool has_dz, int64_t row0, int64_t nrows, int64_t B, int64_t C,
                         void* workspace, size_t workspace_bytes) {
    VIPANT_REQUIRE(B > 0 && C > 0 && B < (1ll << 31) && C < (1ll << 30) && ldz >= C, VIPANT_EBADSHAPE,
                   "%s: bad shape B=%ld C=%ld ldz=%ld", who, (long)B, (long)C, (long)ldz);
    VIPANT_REQUIRE(!has_dz || (ldd >= C && ldd < (1ll << 31)), VIPANT_EBADSHAPE, "%s: ldd=%ld is smaller than C=%ld", who, (long)ldd,
                   (long)C);
    VIPANT_REQUIRE(row0 >= 0 && nrows > 0 && row0 + nrows <= B, VIPANT_EBADSHAPE, "%s: row range [%ld, %ld) outside [0, %ld)", who,
                   (long)row0, (long)(row0 + nrows), (long)B);
    const size_t need = (size_t)(cls_groups(nrows) * 2 * sizeof(float));
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= need, VIPANT_ENOWORKSPACE, "%s: workspace of %zu bytes needed, %zu given",
                   who, need, workspace_bytes);
    return VIPANT_OK;
}

extern "C" int32_t vipant_softmax_ce(const float* z, int64_t ldz, const int64_t* labels, const float* logit_scale, float* loss,
                                     uint16_t* dz, int64_t ldd, float* dscale, int32_t* pred, int64_t row0, int64_t nrows,
                                     float grad_scale, int64_t B, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    int32_t rc = cls_check("softmax_ce", ldz, ldd, dz != nullptr, row0, nrows, B, C, workspace, workspace_bytes);
    if (rc != VIPANT_OK) return rc;
    VIPANT_REQUIRE(z != nullptr && labels != nullptr && logit_scale != nullptr && loss != nullptr, VIPANT_EBADSHAPE,
                   "softmax_ce: z, labels, logit_scale and loss are required");
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    const unsigned groups = (unsigned)cls_groups(nrows);
    const float inv_b = (float)(1.0 / (double)B);
#define CLS_LAUNCH(KK)                                                                                                          \
    hipLaunchKernelGGL(softmax_ce_rows<KK>, dim3(groups), dim3(256), 0, s, z, ldz, labels, logit_scale, (bf16_t*)dz, ldd, pred, \
                       (int)row0, (int)nrows, grad_scale, inv_b, (int)C, part)
    if (C <= 64) CLS_LAUNCH(1);
    else if (C <= 128) CLS_LAUNCH(2);
    else if (C <= 256) CLS_LAUNCH(4);
    else if (C <= 576) CLS_LAUNCH(9);
    else if (C <= 64 * CLS_KMAX) CLS_LAUNCH(CLS_KMAX);
    else CLS_LAUNCH(0);
#undef CLS_LAUNCH
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cls_finish, dim3(1), dim3(256), 0, s, part, (int64_t)groups, 1.0 / (double)B, grad_scale, loss, dscale);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

template <typename TG>
static int32_t bce_launch(const char* who, const float* z, int64_t ldz, const TG* targets, int64_t ldt, const float* logit_scale,
                          float* loss, uint16_t* dz, int64_t ldd, float* dscale, float* prob, int64_t ldp, int64_t row0,
                          int64_t nrows, float grad_scale, int64_t B, int64_t C, void* workspace, size_t workspace_bytes,
                          void* stream) {
    int32_t rc = cls_check(who, ldz, ldd, dz != nullptr, row0, nrows, B, C, workspace, workspace_bytes);
    if (rc != VIPANT_OK) return rc;
    VIPANT_REQUIRE(z != nullptr && targets != nullptr && loss != nullptr && ldt >= C, VIPANT_EBADSHAPE,
                   "%s: z, targets and loss are required (ldt >= C)", who);
    VIPANT_REQUIRE(prob == nullptr || ldp >= C, VIPANT_EBADSHAPE, "%s: ldp=%ld is smaller than C=%ld", who, (long)ldp, (long)C);
    VIPANT_REQUIRE(dscale == nullptr || logit_scale != nullptr, VIPANT_EBADSHAPE, "%s: dscale needs logit_scale", who);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    const unsigned groups = (unsigned)cls_groups(nrows);
    const double inv = 1.0 / ((double)B * (double)C);
    hipLaunchKernelGGL(bce_logits_rows<TG>, dim3(groups), dim3(256), 0, s, z, ldz, targets, ldt, logit_scale, (bf16_t*)dz, ldd, prob,
                       ldp, (int)row0, (int)nrows, grad_scale, (float)inv, (int)C, part);
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(cls_finish, dim3(1), dim3(256), 0, s, part, (int64_t)groups, inv, grad_scale, loss, dscale);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" int32_t vipant_bce_logits(const float* z, int64_t ldz, const uint8_t* targets, int64_t ldt, const float* logit_scale,
                                     float* loss, uint16_t* dz, int64_t ldd, float* dscale, float* prob, int64_t ldp, int64_t row0,
                                     int64_t nrows, float grad_scale, int64_t B, int64_t C, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    return bce_launch<uint8_t>("bce_logits", z, ldz, targets, ldt, logit_scale, loss, dz, ldd, dscale, prob, ldp, row0, nrows, grad_scale,
                               B, C, workspace, workspace_bytes, stream);
}

extern "C" int32_t vipant_bce_logits_soft(const float* z, int64_t ldz, const float* targets, int64_t ldt, const float* logit_scale,
                                          float* loss, uint16_t* dz, int64_t ldd, float* dscale, float* prob, int64_t ldp,
                                          int64_t row0, int64_t nrows, float grad_scale, int64_t B, int64_t C, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    return bce_launch<float>("bce_logits_soft", z, ldz, targets, ldt, logit_scale, loss, dz, ldd, dscale, prob, ldp, row0, nrows,
                             grad_scale, B, C, workspace, workspace_bytes, stream);
}
