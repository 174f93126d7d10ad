// Multi-label hinge tagging loss (BCHingeLossHead, cvap/module/decoder/loss_more.py:145-198): nn.MultiLabelMarginLoss on
// p = sigmoid(s z), s = exp(logit_scale), z the UNSCALED fp32 logits of the head's last Linear, the positives Y of a row being
// the non-zero entries of its multi-hot target (label[i].nonzero(), loss_more.py:161).
//
// The closed form.  With P = |Y|, N = C - P:  row_loss = (1/C) sum_{j in Y} sum_{i not in Y} max(0, 1 - (p_j - p_i)).  p lies in
// [0, 1], so every margin 1 - p_j + p_i is >= 0 and the max never cuts; a margin is exactly 0 only where both sigmoids have
// saturated, and there p (1 - p) = 0 lets no gradient through either way.  The P x N pair walk is therefore, with no approximation,
//   row_loss = ( P N - N sum_{j in Y} p_j + P sum_{i not in Y} p_i ) / C = ( N sum_{j in Y} (1 - p_j) + P sum_{i not in Y} p_i ) / C
//   d row_loss / d p_c = -N / C (c in Y), +P / C (otherwise);   dz_c = grad_scale / B * (d row_loss / d p_c) * p_c (1 - p_c) * s
//   d loss / d logit_scale = sum over rows and classes of dz_c z_c          (the parameter is the log: s = exp(logit_scale))
// and rows with P = 0 or P = C contribute nothing.  The second spelling of row_loss is the one computed: every term is
// non-negative, so a row whose positives all score near 1 loses nothing to P N - N sum p_j.  No index lists, no pairs.
//
// The sigmoid.  With e = exp(-|x|): p = (x >= 0 ? 1 : e) / (1 + e), 1 - p = (x >= 0 ? e : 1) / (1 + e) -- no overflow, both
// limits exact, no cancellation on either side.  x = s z, e, p, 1 - p and p (1 - p) are formed in fp64 and rounded once each.  Two
// reasons, both about the last places of the scores.  On the saturated side p (or 1 - p) is e, whose RELATIVE error is the ABSOLUTE
// error of x, and an fp32 product s z is off by up to |x| 2^-24 -- 40 units in the last place of p at x = -40.  And 1 + e lies in
// [1, 2) where fp32 is half as fine as in [0.5, 1): rounding it alone moves p = 1 / (1 + e) by a unit of p's last place, and the
// fp32 form ends just above 2 units.  The row's sums, the gradient and everything after are fp32; the row costs one fp64 exp and one
// fp64 division per class, which a kernel of one wave per row that waits on its loads does not notice.
//
// Layout: one wave per row, HNG_WAVES rows per workgroup, lane l owns classes l + 64 t.  A row of C <= 64 K classes (K = 1, 2, 4,
// 9, 16 by a table) stays in registers between the two phases: per class p (1 - p) and x, the target marks as one bit mask; z and
// the targets are read once.  Phase 1: P, sum_{Y} (1 - p), sum_{not Y} p, and the scores `prob`.  Phase 2: dz and
// the row's dscale term.  Wider rows (K = 0) take the same two phases with phase 2 reading z and the targets again.  Row sums stay
// inside the wave: four DPP steps leave each 16-lane row's sum in its lanes, the four rows are added in row order from
// readlanes (wave-uniform).  dz is bf16: an even lane fetches its right neighbour's value with one DPP move and stores the
// pair as 32 bits where the row's address allows; an unaligned row and the last column of an odd ldd are stored one by one.
//
// Each wave writes its row's two partials (loss, dscale) to workspace[2 * row]; hinge_fold adds them in fp64 in a fixed order.
// No atomics, no barrier in the row kernel, every workspace word that is read was written by the same call: two runs give the
// same bits whatever the workspace held.
#include "common.h"

#define HNG_WAVES 4      // rows per workgroup
#define HNG_KMAX 16      // register-resident rows: C <= 64 * HNG_KMAX

// sum over the wave, the same bits in every lane (all 64 lanes active); T = float or int
template <int CTRL, typename T>
__device__ __forceinline__ T hng_dpp_add(T v) {
    return v + __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <typename T>
__device__ __forceinline__ T hng_wave_sum(T v) {
    v = hng_dpp_add<0xB1>(v);       // quad_perm [1, 0, 3, 2]
    v = hng_dpp_add<0x4E>(v);       // quad_perm [2, 3, 0, 1]
    v = hng_dpp_add<0x141>(v);      // row_half_mirror: the other quad of the eight
    v = hng_dpp_add<0x140>(v);      // row_mirror: the other eight of the sixteen
    const int b = __builtin_bit_cast(int, v);
    const T r0 = __builtin_bit_cast(T, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(T, __builtin_amdgcn_readlane(b, 16));
    const T r2 = __builtin_bit_cast(T, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(T, __builtin_amdgcn_readlane(b, 48));
    return ((r0 + r1) + r2) + r3;
}

struct HngElem {
    float p, q, w, x;      // sigmoid(x), 1 - sigmoid(x), their product, x = s z
};
__device__ __forceinline__ HngElem hng_elem(float z, double s) {
    const double xd = s * (double)z;
    const double e = exp(-fabs(xd));            // in [0, 1]
    const double r = 1.0 / (1.0 + e), er = e * r;
    const double pd = xd >= 0.0 ? r : er, qd = xd >= 0.0 ? er : r;
    return {(float)pd, (float)qd, (float)(pd * qd), (float)xd};
}

// K > 0: the row's K x 64 classes stay in registers between the phases; K == 0: phase 2 reads memory again
template <int K, typename TG>
__global__ __launch_bounds__(64 * HNG_WAVES) void hinge_rows(const float* __restrict__ z, int64_t ldz, const TG* __restrict__ tg, int64_t ldt,
                                                             const float* __restrict__ logit_scale, bf16_t* __restrict__ dz, int64_t ldd,
                                                             float* __restrict__ prob, int64_t ldp, int row0, int nrows, float grad_scale,
                                                             float inv_b, int C, float* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int local = blockIdx.x * HNG_WAVES + (threadIdx.x >> 6);
    if (local >= nrows) return;                                   // whole waves leave; the kernel has no barrier
    const int64_t row = (int64_t)row0 + local;
    const double s = logit_scale != nullptr ? exp((double)logit_scale[0]) : 1.0;
    const float* zr = z + row * ldz;
    const TG* tr = tg + row * ldt;
    float* prow = prob != nullptr ? prob + row * ldp : nullptr;
    const int n = K > 0 ? K : (C + 63) >> 6;

    // ---- phase 1: the scores, the marks, the three row sums
    constexpr int KR = K > 0 ? K : 1;
    float w[KR], xs[KR];          // p (1 - p) and x of class lane + 64 k (0 past C)
    uint32_t marks = 0;           // bit k: class lane + 64 k is a positive
    int P = 0;                    // this lane's positives, then the row's
    float sq = 0.f, sn = 0.f;     // sum_{Y} (1 - p), sum_{not Y} p
#pragma unroll KR
    for (int k = 0; k < n; ++k) {
        const int j = k * 64 + lane;
        bool m = false;
        HngElem v = {0.f, 0.f, 0.f, 0.f};
        if (j < C) {
            m = tr[j] != 0;
            v = hng_elem(zr[j], s);
            if (prow != nullptr) prow[j] = v.p;
            if (m) sq += v.q;
            else sn += v.p;
        }
        P += m;
        if constexpr (K > 0) {
            w[k] = v.w;
            xs[k] = v.x;
            marks |= (uint32_t)m << k;
        }
    }
    P = hng_wave_sum(P);
    sq = hng_wave_sum(sq);
    sn = hng_wave_sum(sn);
    const int N = C - P;
    const float fc = (float)C;
    const float cpos = -(float)N / fc, cneg = (float)P / fc;      // d row_loss / d p_c
    const float g = grad_scale * (float)s * inv_b;

    // ---- phase 2: dz and the row's dscale term
    bf16_t* drow = dz != nullptr ? dz + row * ldd : nullptr;
    const bool pairs = ((uintptr_t)drow & 3) == 0;                // class 64 k + an even lane then sits on a 4-byte boundary
    float dls = 0.f;
#pragma unroll KR
    for (int k = 0; k < n; ++k) {
        const int j = k * 64 + lane;
        float wk = 0.f, xk = 0.f;
        bool m = false;
        if constexpr (K > 0) {
            wk = w[k];
            xk = xs[k];
            m = (marks >> k) & 1u;
        } else if (j < C) {
            const HngElem v = hng_elem(zr[j], s);
            wk = v.w;
            xk = v.x;
            m = tr[j] != 0;
        }
        const float t = (m ? cpos : cneg) * wk;                   // 0 past C: the pad columns of dz are written as zeros
        dls = __builtin_fmaf(t, xk, dls);
        if (drow != nullptr) {
            const uint32_t own = __builtin_bit_cast(uint16_t, f32_to_bf16(g * t));
            const uint32_t right = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xf, 0xf, false);      // lane ^ 1
            if (pairs && (lane & 1) == 0 && j + 1 < ldd) *(uint32_t*)(drow + j) = own | (right << 16);
            else if (j < ldd && !(pairs && (lane & 1))) drow[j] = __builtin_bit_cast(bf16_t, (uint16_t)own);
        }
    }
    if (drow != nullptr)
        for (int64_t j = (int64_t)n * 64 + lane; j < ldd; j += 64) drow[j] = f32_to_bf16(0.f);
    dls = hng_wave_sum(dls);
    if (lane == 0) {
        part[2 * (int64_t)local] = ((float)N * sq + (float)P * sn) / fc;
        part[2 * (int64_t)local + 1] = dls;
    }
}

// one workgroup adds the per-row partials in index order (fp64): loss = sum / B, dscale = grad_scale * sum / B
__global__ __launch_bounds__(256) void hinge_fold(const float* __restrict__ part, int64_t nrows, double inv_b, float grad_scale,
                                                  float* __restrict__ loss, float* __restrict__ dscale) {
    __shared__ double red[2][256];
    double a = 0.0, b = 0.0;
    for (int64_t t = threadIdx.x; t < nrows; t += 256) {
        a += (double)part[2 * t];
        b += (double)part[2 * t + 1];
    }
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(red[0][0] * inv_b);
        if (dscale != nullptr) dscale[0] = (float)((double)grad_scale * red[1][0] * inv_b);
    }
}

// ---- host entry points ------------------------------------------------------------------------------------------------
extern "C" size_t vipant_hinge_logits_workspace_bytes(int64_t nrows) { return (size_t)(nrows > 0 ? nrows : 1) * 2 * sizeof(float); }

template <typename TG>
static void hinge_launch(const float* z, int64_t ldz, const TG* tg, int64_t ldt, const float* logit_scale, bf16_t* dz, int64_t ldd, float* prob,
                         int64_t ldp, int row0, int nrows, float grad_scale, float inv_b, int C, float* part, hipStream_t s) {
    const unsigned groups = (unsigned)ceil_div(nrows, HNG_WAVES);
#define HNG_LAUNCH(KK)                                                                                                                  \
    hipLaunchKernelGGL((hinge_rows<KK, TG>), dim3(groups), dim3(64 * HNG_WAVES), 0, s, z, ldz, tg, ldt, logit_scale, dz, ldd, prob, ldp, \
                       row0, nrows, grad_scale, inv_b, C, part)
    if (C <= 64) HNG_LAUNCH(1);
    else if (C <= 128) HNG_LAUNCH(2);
    else if (C <= 256) HNG_LAUNCH(4);
    else if (C <= 576) HNG_LAUNCH(9);
    else if (C <= 64 * HNG_KMAX) HNG_LAUNCH(HNG_KMAX);
    else HNG_LAUNCH(0);
#undef HNG_LAUNCH
}

extern "C" int32_t vipant_hinge_logits(const float* z, int64_t ldz, const void* targets, int64_t ldt, int32_t target_kind,
                                       const float* logit_scale, float* loss, uint16_t* dz, int64_t ldd, float* dscale, float* prob,
                                       int64_t ldp, int64_t row0, int64_t nrows, float grad_scale, int64_t B, int64_t C, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    // the shapes vipant_bce_logits takes (classify.hip: cls_check), refused before any launch
    VIPANT_REQUIRE(B > 0 && C > 0 && B < (1ll << 31) && C < (1ll << 30) && ldz >= C, VIPANT_EBADSHAPE,
                   "hinge_logits: bad shape B=%ld C=%ld ldz=%ld", (long)B, (long)C, (long)ldz);
    VIPANT_REQUIRE(dz == nullptr || (ldd >= C && ldd < (1ll << 31)), VIPANT_EBADSHAPE, "hinge_logits: ldd=%ld is smaller than C=%ld",
                   (long)ldd, (long)C);
    VIPANT_REQUIRE(row0 >= 0 && nrows > 0 && row0 + nrows <= B, VIPANT_EBADSHAPE, "hinge_logits: row range [%ld, %ld) outside [0, %ld)",
                   (long)row0, (long)(row0 + nrows), (long)B);
    VIPANT_REQUIRE(target_kind == 0 || target_kind == 1, VIPANT_EBADSHAPE, "hinge_logits: target_kind=%d is neither 0 (uint8) nor 1 (fp32)",
                   (int)target_kind);
    VIPANT_REQUIRE(z != nullptr && targets != nullptr && loss != nullptr && ldt >= C, VIPANT_EBADSHAPE,
                   "hinge_logits: z, targets and loss are required (ldt >= C)");
    VIPANT_REQUIRE(prob == nullptr || ldp >= C, VIPANT_EBADSHAPE, "hinge_logits: ldp=%ld is smaller than C=%ld", (long)ldp, (long)C);
    VIPANT_REQUIRE(dscale == nullptr || logit_scale != nullptr, VIPANT_EBADSHAPE, "hinge_logits: dscale needs logit_scale");
    const size_t need = vipant_hinge_logits_workspace_bytes(nrows);
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= need, VIPANT_ENOWORKSPACE, "hinge_logits: workspace of %zu bytes needed, %zu given",
                   need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)workspace;
    const double inv_b = 1.0 / (double)B;
    if (target_kind == 0)
        hinge_launch<uint8_t>(z, ldz, (const uint8_t*)targets, ldt, logit_scale, (bf16_t*)dz, ldd, prob, ldp, (int)row0, (int)nrows, grad_scale,
                              (float)inv_b, (int)C, part, s);
    else
        hinge_launch<float>(z, ldz, (const float*)targets, ldt, logit_scale, (bf16_t*)dz, ldd, prob, ldp, (int)row0, (int)nrows, grad_scale,
                            (float)inv_b, (int)C, part, s);
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(hinge_fold, dim3(1), dim3(256), 0, s, part, nrows, inv_b, grad_scale, loss, dscale);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}
