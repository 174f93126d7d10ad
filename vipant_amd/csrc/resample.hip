// Sample-rate conversion (gfx950, wave64): a ragged batch of fp32 waveforms [b, wave_stride], each clip at its own rate, in; the same
// clips at ONE rate [b, out_stride] out, in one launch.  It is the stage between `vipant_pcm_ingest` and the log-mel launch that the
// reference does not have (it takes each file at its own rate, cvap/data/audio/transform.py:15-35) and that every PyTorch audio
// pipeline applies as torchaudio.functional.resample(waveform, orig, new) at its defaults: band-limited polyphase interpolation with
// a Hann-windowed sinc.  For g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * rolloff, L = lowpass_filter_width,
// w = ceil(L * o / base), phase j = 0 .. n-1 and tap k = 0 .. 2w + o - 1:
//     t      = clamp((-j / n + (k - w) / o) * base, -L, L)
//     K[j,k] = (t == 0 ? 1 : sin(pi t) / (pi t)) * cos^2(pi t / (2 L)) * base / o          in fp64, rounded once to fp32
//     out[i n + j] = sum_k K[j,k] * x[i o + k - w]          (x = 0 outside [0, len)),   len_out = ceil(n * len / o)
// A tap with |t| >= L before the clamp is 1e-49 in fp64 and exactly 0 in fp32, so the table keeps, per phase, the run of taps with
// |t| < L: it starts at k0[j] and has at most T taps (34 of 475 for 44100 -> 16000), zero filled where a phase has fewer.
//
// resample_table_kernel   builds one rate pair's table on the device: coef fp32 [T][n] (transposed: lanes that own consecutive phases
//                         read consecutive words), then k0 int32 [n].  fp64 arithmetic, one rounding.  k0[j] is found from the
//                         same fp64 expression for t on the host (the plan: T, the range of k0) and on the device; division,
//                         multiplication and addition are IEEE on both and the expression holds no multiply-add to contract.
// resample_kernel         grid (output blocks, clips).  A clip's class -- its rate pair -- is a byte in the launch's argument block
//                         and indexes the class descriptors beside it: nothing is copied to the device for a call and nothing is
//                         waited for.  A workgroup of 256 threads owns P consecutive periods i0 .. i0 + P - 1 of one clip = P n
//                         consecutive outputs.  It stages the class's table and the input span those periods read,
//                         (P - 1) o + (max k0 - min k0) + T samples from i0 o + min k0 - w, into LDS once: 16-byte loads on the
//                         global side's own alignment (the LDS copy starts up to 3 samples early so that both sides are aligned),
//                         and every index outside [0, len) becomes 0 without being read -- the padding of a row may hold anything.
//                         A thread owns one phase j and R = 4 periods g, g + G, g + 2G, g + 3G (G = P / 4): item q = g n + j is the
//                         flattened output index inside the first G periods, so 256 lanes are busy for any n (1, 2, 147, 640) and
//                         the four stores of an item are four fully coalesced rows of the workgroup.  Per tap: ONE coefficient
//                         read and four input reads for four FMAs (1.25 LDS reads per FMA; phase by phase it would be 2).
//                         Accumulation: fp32 FMA in ascending k from +0 -- an output's bits depend on its clip alone, not on P,
//                         the batch or the run.  Outputs from len_out to out_stride are written as 0, nsamples_out = len_out.
//                         The identity class (orig == new) is a copy in the same launch, bit for bit.
// No matrix instructions: the operands need fp32 grade (audio lives at 16+ bits; gfx950 has no MFMA with fp32 operands) and the dense
// [n, 2w + o] form would spend 14 x the multiply-adds on zeros.
#include <math.h>
#include <string.h>

#include "common.h"

namespace {

constexpr int RS_THREADS = 256, RS_R = 4;
constexpr int RS_CHUNK = 2048;                       // clips per launch: their class bytes travel in the argument block
constexpr int RS_LDS_MAX = 160 * 1024;               // the LDS of a workgroup
constexpr int RS_LDS_GOAL = 64 * 1024;               // what the plan aims at: two workgroups per CU
constexpr int RS_BLOCK_OUTPUTS = 4096;               // P n of the plan, at most
constexpr int RS_FIELD_MAX = 65535;                  // n and T of a descriptor
constexpr int64_t RS_LIM = (int64_t)1 << 40;

// ---- the filter, shared by the host's plan and the device's table -------------------------------------------------------------------
struct RsFilter { int o, n, w; double base, L; };

__host__ __device__ inline double rs_t(const RsFilter& f, int64_t j, int64_t k) {
    return (-(double)j / (double)f.n + (double)(k - f.w) / (double)f.o) * f.base;
}
// the first tap of phase j with t > -L (t grows with k): a closed-form guess, corrected by the expression itself
__host__ __device__ inline int rs_k0(const RsFilter& f, int64_t j) {
    const int64_t kend = 2 * (int64_t)f.w + f.o;
    int64_t k = f.w + (int64_t)floor((double)j * (double)f.o / (double)f.n - f.L * (double)f.o / f.base);
    k = k < 0 ? 0 : (k > kend ? kend : k);
    while (k > 0 && rs_t(f, j, k - 1) > -f.L) --k;
    while (k < kend && rs_t(f, j, k) <= -f.L) ++k;
    return (int)k;
}
// the first tap of phase j with t >= L, or 2w + o
__host__ __device__ inline int rs_k1(const RsFilter& f, int64_t j) {
    const int64_t kend = 2 * (int64_t)f.w + f.o;
    int64_t k = f.w + (int64_t)ceil((double)j * (double)f.o / (double)f.n + f.L * (double)f.o / f.base);
    k = k < 0 ? 0 : (k > kend ? kend : k);
    while (k < kend && rs_t(f, j, k) < f.L) ++k;
    while (k > 0 && rs_t(f, j, k - 1) >= f.L) --k;
    return (int)k;
}

int64_t rs_gcd(int64_t a, int64_t b) {
    while (b) {
        const int64_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

inline int64_t rs_up4(int64_t v) { return (v + 3) & ~(int64_t)3; }
// LDS of one workgroup in bytes: the table, then the staged span (3 more samples for the alignment shift, rounded up to a quad)
inline int64_t rs_lds_bytes(int64_t n, int64_t T, int64_t o, int64_t kspan, int64_t P) {
    return (rs_up4((T + 1) * n) + rs_up4((P - 1) * o + kspan + 3)) * 4;
}

// the rate pair's filter and, in *c, everything of its descriptor but the table pointer -> 0, or a refusal (vipant_last_error is set)
int32_t rs_plan(int64_t orig, int64_t fresh, int32_t width, double rolloff, RsFilter* f, vipant_resample_class* c) {
    VIPANT_REQUIRE(orig >= 1 && fresh >= 1 && orig < ((int64_t)1 << 31) && fresh < ((int64_t)1 << 31), VIPANT_EBADSHAPE,
                   "resample: rates (%lld, %lld) outside [1, 2^31)", (long long)orig, (long long)fresh);
    VIPANT_REQUIRE(width >= 1 && width <= 64 && rolloff > 0.0 && rolloff <= 1.0, VIPANT_EBADSHAPE,
                   "resample: lowpass_filter_width = %d outside [1, 64] or rolloff = %g outside (0, 1]", (int)width, rolloff);
    const int64_t g = rs_gcd(orig, fresh), o = orig / g, n = fresh / g;
    memset(c, 0, sizeof(*c));
    c->orig = (int32_t)orig;
    c->fresh = (int32_t)fresh;
    if (o == n) {                                     // the identity class: a copy
        c->o = c->n = 1;
        c->P = RS_BLOCK_OUTPUTS;
        return VIPANT_OK;
    }
    VIPANT_REQUIRE(n <= RS_FIELD_MAX && o < ((int64_t)1 << 24), VIPANT_EBADSHAPE,
                   "resample: %lld -> %lld Hz has %lld phases of step %lld; a class descriptor holds at most %d phases "
                   "(rates that share a large divisor, such as 44100 and 16000, have few)",
                   (long long)orig, (long long)fresh, (long long)n, (long long)o, RS_FIELD_MAX);
    const double base = (double)(o < n ? o : n) * rolloff;
    const double wd = ceil((double)width * (double)o / base);
    VIPANT_REQUIRE(wd < (double)(1 << 24), VIPANT_EBADSHAPE, "resample: %lld -> %lld Hz: filter half-width out of range",
                   (long long)orig, (long long)fresh);
    *f = RsFilter{(int)o, (int)n, (int)wd, base, (double)width};
    int64_t T = 0, kmin = INT64_MAX, kmax = 0;
    for (int64_t j = 0; j < n; ++j) {
        const int64_t k0 = rs_k0(*f, j), k1 = rs_k1(*f, j);
        T = k1 - k0 > T ? k1 - k0 : T;
        kmin = k0 < kmin ? k0 : kmin;
        kmax = k0 > kmax ? k0 : kmax;
    }
    const int64_t kspan = kmax - kmin + T;
    VIPANT_REQUIRE(T >= 1 && T <= RS_FIELD_MAX, VIPANT_EBADSHAPE,
                   "resample: %lld -> %lld Hz needs %lld taps per phase; a class descriptor holds at most %d", (long long)orig,
                   (long long)fresh, (long long)T, RS_FIELD_MAX);
    // P: a multiple of R with P n <= RS_BLOCK_OUTPUTS, shrunk until table + span fit RS_LDS_GOAL; where not even P = R fits the
    // workgroup's LDS, 3, 2 or 1 periods with one period per thread
    int64_t P = RS_BLOCK_OUTPUTS / n / RS_R * RS_R;
    P = P < RS_R ? RS_R : P;
    if (rs_lds_bytes(n, T, o, kspan, P) > RS_LDS_GOAL) {
        const int64_t room = RS_LDS_GOAL / 4 - rs_up4((T + 1) * n) - rs_up4(kspan + 3) - 4;
        const int64_t fit = room > 0 ? (room / o + 1) / RS_R * RS_R : 0;
        P = fit < RS_R ? RS_R : (fit < P ? fit : P);
    }
    while (P > 1 && rs_lds_bytes(n, T, o, kspan, P) > RS_LDS_MAX) P = P > RS_R ? P - RS_R : P - 1;
    const int64_t bytes = rs_lds_bytes(n, T, o, kspan, P);
    VIPANT_REQUIRE(bytes <= RS_LDS_MAX, VIPANT_EBADSHAPE,
                   "resample: %lld -> %lld Hz needs %lld bytes of LDS (a table of %lld phases x %lld taps and one period's span); a "
                   "workgroup has %d", (long long)orig, (long long)fresh, (long long)bytes, (long long)n, (long long)T, RS_LDS_MAX);
    c->o = (int32_t)o;
    c->n = (int32_t)n;
    c->T = (int32_t)T;
    c->w = f->w;
    c->P = (int32_t)P;
    c->kmin = (int32_t)kmin;
    c->kspan = (int32_t)kspan;
    c->lds_bytes = (int32_t)bytes;
    return VIPANT_OK;
}

// ---- the table ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void resample_table_kernel(float* __restrict__ table, RsFilter f, int T) {
    const int64_t total = (int64_t)(T + 1) * f.n;
    const int64_t e = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (e >= total) return;
    const int kk = (int)(e / f.n), j = (int)(e - (int64_t)kk * f.n);
    const int k0 = rs_k0(f, j);
    if (kk == T) {
        ((int32_t*)table)[e] = k0;
        return;
    }
    const int64_t k = (int64_t)k0 + kk;
    const double t = rs_t(f, j, k);
    float v = 0.f;                                    // a phase with fewer than T taps: zeros behind its run
    if (k < 2 * (int64_t)f.w + f.o && t < f.L) {      // (t > -L from k0 on)
        const double tp = t * M_PI, c = cos(tp / (2.0 * f.L));
        v = (float)((t == 0.0 ? 1.0 : sin(tp) / tp) * (c * c) * f.base / (double)f.o);
    }
    table[e] = v;
}

// ---- the launch's argument block ----------------------------------------------------------------------------------------------------
struct RsArgs {
    vipant_resample_class cls[VIPANT_RESAMPLE_MAX_CLASSES];
    uint8_t idx[RS_CHUNK];
};

template <int R>
__device__ __forceinline__ void rs_periods(const float* __restrict__ coef, const int32_t* __restrict__ k0s, const float* __restrict__ xs,
                                           float* __restrict__ orow, int64_t e0, int64_t e1, int64_t len_out, int o, int n, int T, int P,
                                           int kmin, int klast) {
    const int G = P / R, items = G * n, hop = G * o;
    const int64_t row = (int64_t)G * n;
    for (int q = threadIdx.x; q < items; q += RS_THREADS) {
        const int g = q / n, j = q - g * n;
        int k0 = k0s[j];
        k0 = k0 < kmin ? kmin : (k0 > klast ? klast : k0);            // whatever the table says, no read leaves the staged span
        const float* xp = xs + g * o + (k0 - kmin);
        const float* cp = coef + j;
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
#pragma unroll 4
        for (int k = 0; k < T; ++k) {
            const float c = cp[(int64_t)k * n];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(c, xp[r * hop + k], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t e = e0 + q + r * row;
            if (e < e1) orow[e] = e < len_out ? acc[r] : 0.f;
        }
    }
}

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ wave, int64_t wave_stride,
                                                               const int64_t* __restrict__ nsamples, float* __restrict__ out,
                                                               int64_t out_stride, int64_t* __restrict__ nsamples_out, const RsArgs a) {
    extern __shared__ f32x4 rs_lds[];
    const int64_t clip = blockIdx.y;
    const vipant_resample_class& c = a.cls[a.idx[clip]];
    const int o = c.o, n = c.n, T = c.T, P = c.P;
    const int64_t block = (int64_t)P * n, e0 = (int64_t)blockIdx.x * block;
    if (e0 >= out_stride) return;
    const int64_t e1 = e0 + block < out_stride ? e0 + block : out_stride;
    int64_t len = nsamples[clip];
    len = len < 0 ? 0 : (len > wave_stride ? wave_stride : len);                // a device value: clamped, not refused
    int64_t len_out = (len * n + o - 1) / o;
    len_out = len_out < out_stride ? len_out : out_stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) nsamples_out[clip] = len_out;
    const float* xrow = wave + clip * wave_stride;
    float* orow = out + clip * out_stride;
    if (e0 >= len_out) {                                                        // past the clip: its share of the row's zeros
        for (int64_t e = e0 + threadIdx.x; e < e1; e += RS_THREADS) orow[e] = 0.f;
        return;
    }
    if (T == 0) {                                                               // the identity class: quads on the output's alignment
        const int head = (int)((4 - (((uintptr_t)(orow + e0) >> 2) & 3)) & 3);
        const int64_t q0 = e0 + head < e1 ? e0 + head : e1, nq = (e1 - q0) / 4;
        for (int64_t e = e0 + threadIdx.x; e < q0; e += RS_THREADS) orow[e] = e < len ? xrow[e] : 0.f;
        for (int64_t q = threadIdx.x; q < nq; q += RS_THREADS) {
            const int64_t e = q0 + 4 * q;
            f32x4 v;
            if (e + 4 <= len && ((uintptr_t)(xrow + e) & 15) == 0) {
                v = *(const f32x4*)(xrow + e);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = e + u < len ? xrow[e + u] : 0.f;
            }
            *(f32x4*)(orow + e) = v;
        }
        for (int64_t e = q0 + 4 * nq + threadIdx.x; e < e1; e += RS_THREADS) orow[e] = e < len ? xrow[e] : 0.f;
        return;
    }
    float* lds = (float*)rs_lds;
    const int64_t words = (int64_t)(T + 1) * n;
    float* xs = lds + ((words + 3) & ~(int64_t)3);
    {                                                                           // the class's table: 16-byte words, then its tail
        const f32x4* t4 = (const f32x4*)c.table;
        const int64_t nq = words / 4;
        for (int64_t q = threadIdx.x; q < nq; q += RS_THREADS) rs_lds[q] = t4[q];
        for (int64_t e = 4 * nq + threadIdx.x; e < words; e += RS_THREADS) lds[e] = ((const float*)c.table)[e];
    }
    const int64_t s0 = (int64_t)blockIdx.x * P * o + c.kmin - c.w;            // the first sample the block's periods read
    const int mis = (int)((((int64_t)((uintptr_t)xrow >> 2)) + s0) & 3);        // s0's distance from a 16-byte boundary of the row
    {
        const int64_t s0a = s0 - mis;
        const int nq = ((P - 1) * o + c.kspan + mis + 3) / 4;
        for (int q = threadIdx.x; q < nq; q += RS_THREADS) {
            const int64_t e = s0a + 4 * (int64_t)q;
            f32x4 v;
            if (e >= 0 && e + 4 <= len) {
                v = *(const f32x4*)(xrow + e);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = (e + u >= 0 && e + u < len) ? xrow[e + u] : 0.f;
            }
            *(f32x4*)(xs + 4 * q) = v;
        }
    }
    __syncthreads();
    const int klast = c.kmin + c.kspan - T;
    if (P % RS_R == 0)
        rs_periods<RS_R>(lds, (const int32_t*)(lds + (int64_t)T * n), xs + mis, orow, e0, e1, len_out, o, n, T, P, c.kmin, klast);
    else
        rs_periods<1>(lds, (const int32_t*)(lds + (int64_t)T * n), xs + mis, orow, e0, e1, len_out, o, n, T, P, c.kmin, klast);
}

bool rs_class_ok(const vipant_resample_class& c) {
    if (c.T == 0) return c.o == 1 && c.n == 1 && c.P >= 1 && (int64_t)c.P <= RS_BLOCK_OUTPUTS;
    return c.table != nullptr && ((uintptr_t)c.table & 15) == 0 && c.o >= 1 && c.n >= 1 && c.n <= RS_FIELD_MAX && c.T >= 1 &&
           c.T <= RS_FIELD_MAX && c.P >= 1 && c.w >= 0 && c.kmin >= 0 && c.kspan >= c.T &&
           rs_lds_bytes(c.n, c.T, c.o, c.kspan, c.P) <= RS_LDS_MAX;
}

}  // namespace

extern "C" int32_t vipant_resample_plan(int64_t orig, int64_t fresh, int32_t lowpass_filter_width, double rolloff,
                                        vipant_resample_class* cls) {
    VIPANT_REQUIRE(cls, VIPANT_EBADSHAPE, "resample_plan: NULL argument");
    RsFilter f{};
    return rs_plan(orig, fresh, lowpass_filter_width, rolloff, &f, cls);
}

extern "C" size_t vipant_resample_table_bytes(int64_t orig, int64_t fresh, int32_t lowpass_filter_width, double rolloff) {
    RsFilter f{};
    vipant_resample_class c;
    if (rs_plan(orig, fresh, lowpass_filter_width, rolloff, &f, &c) != VIPANT_OK) return 0;
    return (size_t)(c.T ? (int64_t)(c.T + 1) * c.n * 4 : 0);
}

extern "C" int32_t vipant_resample_table(int64_t orig, int64_t fresh, int32_t lowpass_filter_width, double rolloff, void* table,
                                         size_t bytes, void* stream) {
    RsFilter f{};
    vipant_resample_class c;
    const int32_t rc = rs_plan(orig, fresh, lowpass_filter_width, rolloff, &f, &c);
    if (rc != VIPANT_OK) return rc;
    if (c.T == 0) return VIPANT_OK;                                            // the identity class has no table
    const int64_t words = (int64_t)(c.T + 1) * c.n;
    VIPANT_REQUIRE(table && ((uintptr_t)table & 15) == 0, VIPANT_EALIGN, "resample_table: table must be a 16-byte aligned pointer");
    VIPANT_REQUIRE(bytes >= (size_t)words * 4, VIPANT_ENOWORKSPACE, "resample_table: %lld -> %lld Hz needs %lld bytes, got %zu",
                   (long long)orig, (long long)fresh, (long long)words * 4, bytes);
    hipLaunchKernelGGL(resample_table_kernel, dim3((unsigned)ceil_div(words, RS_THREADS)), dim3(RS_THREADS), 0, (hipStream_t)stream,
                       (float*)table, f, (int)c.T);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" int32_t vipant_resample(const float* wave, int64_t wave_stride, const int64_t* nsamples, const int32_t* cls,
                                   const vipant_resample_class* classes, int32_t nclasses, float* out, int64_t out_stride,
                                   int64_t* nsamples_out, int64_t b, void* stream) {
    VIPANT_REQUIRE(wave && nsamples && cls && classes && out && nsamples_out, VIPANT_EBADSHAPE, "resample: NULL argument");
    VIPANT_REQUIRE(b >= 1 && b < ((int64_t)1 << 20), VIPANT_EBADSHAPE, "resample: b = %lld outside [1, 2^20)", (long long)b);
    VIPANT_REQUIRE(wave_stride >= 1 && wave_stride < RS_LIM && out_stride >= 1 && out_stride < RS_LIM, VIPANT_EBADSHAPE,
                   "resample: strides (%lld, %lld) outside [1, 2^40)", (long long)wave_stride, (long long)out_stride);
    VIPANT_REQUIRE(nclasses >= 1 && nclasses <= VIPANT_RESAMPLE_MAX_CLASSES, VIPANT_EBADSHAPE, "resample: %d classes outside [1, %d]",
                   (int)nclasses, VIPANT_RESAMPLE_MAX_CLASSES);
    const uintptr_t w0 = (uintptr_t)wave, w1 = w0 + (uintptr_t)(b * wave_stride) * 4, o0 = (uintptr_t)out,
                    o1 = o0 + (uintptr_t)(b * out_stride) * 4;
    VIPANT_REQUIRE(o1 <= w0 || w1 <= o0, VIPANT_EBADSHAPE, "resample: out overlaps wave (the launch reads a span per output block)");
    for (int32_t k = 0; k < nclasses; ++k)
        VIPANT_REQUIRE(rs_class_ok(classes[k]), VIPANT_EBADSHAPE, "resample: class %d is not a descriptor of vipant_resample_plan with its table", (int)k);
    for (int64_t i = 0; i < b; ++i)
        VIPANT_REQUIRE(cls[i] >= 0 && cls[i] < nclasses, VIPANT_EBADSHAPE, "resample: clip %lld has class %d outside [0, %d)", (long long)i,
                       (int)cls[i], (int)nclasses);
    static DeviceMax most;
    for (int64_t first = 0; first < b; first += RS_CHUNK) {                    // one launch up to 2048 clips
        const int64_t count = b - first < RS_CHUNK ? b - first : RS_CHUNK;
        RsArgs a;
        memset(&a, 0, sizeof(a));
        for (int32_t k = 0; k < nclasses; ++k) a.cls[k] = classes[k];
        int lds = 0;
        int64_t blocks = 1;
        for (int64_t i = 0; i < count; ++i) {
            const vipant_resample_class& c = classes[cls[first + i]];
            a.idx[i] = (uint8_t)cls[first + i];
            const int need = c.T ? (int)rs_lds_bytes(c.n, c.T, c.o, c.kspan, c.P) : 0;
            lds = need > lds ? need : lds;
            const int64_t nb = ceil_div(out_stride, (int64_t)c.P * c.n);
            blocks = nb > blocks ? nb : blocks;
        }
        VIPANT_REQUIRE(blocks < ((int64_t)1 << 31), VIPANT_EBADSHAPE, "resample: %lld output blocks per clip", (long long)blocks);
        if (lds > 64 * 1024 && raise_on_device(most, lds)) {
            VIPANT_HIP_TRY(hipFuncSetAttribute((const void*)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            raised_on_device(most, lds);
        }
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks, (unsigned)count), dim3(RS_THREADS), lds, (hipStream_t)stream,
                           wave + first * wave_stride, wave_stride, nsamples + first, out + first * out_stride, out_stride,
                           nsamples_out + first, a);
        VIPANT_LAUNCH_CHECK();
    }
    return VIPANT_OK;
}
