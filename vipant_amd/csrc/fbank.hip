// Log-mel front-end on the GPU: the Kaldi-style filter bank the reference computes per clip on CPU dataloader workers
// (cvap/data/audio/transform.py:12-35 -> torchaudio.compliance.kaldi.fbank with the parameters of
// cvap/data/image_audio.py:119-126), followed by the dataset's zero padding, (x - mean) / std and SpecAugment
// masks (image_audio.py:183-207).  Output is the [b, 1, T, F] fp32 spectrogram batch the audio tower consumes, so the
// waveform never leaves the device once it is there.
//
// One wave per frame PAIR (two real frames packed into one complex transform), four waves per workgroup, each walking
// four pairs (the workgroup's tables serve 32 frames).  A frame is framed (snip_edges), DC-removed, pre-emphasised
// (replicated first sample), windowed and zero-padded to NFFT in LDS; a radix-2 Stockham FFT (log2 NFFT passes
// ping-ponging two LDS buffers, twiddles from sincospi -- exact at the power-of-two fractions) gives the spectrum;
// every lane then owns mel bins lane, lane + 64, ... and sums power x weight over that filter's (contiguous)
// support; log with the epsilon floor, normalisation and masks are applied on the way out (coalesced row stores).
// HBM traffic = waveform read (overlapping frames hit L2) + b*T*F*4 B written: the kernel is launch/HBM bound, the
// FFT is ~25 kFLOP per frame.
#include "common.h"

namespace {

struct FbankArgs {
    const float* wave; int64_t wave_stride; const int64_t* nsamples; float* out;
    const float* window; const float* banks; const int32_t* bank_start; const int32_t* bank_len; const int32_t* masks;
    const float* clip_mean;
    union { const int32_t* mix_index; const struct ViewPlan* plan; };               // vipant_fbank_mix / vipant_fbank_view only
    const float* mix_lambda; const float* mix_mean;                                // vipant_fbank_mix only
    int T, F, size, shift;
    float preemph, norm_mean, norm_std;
    float* out2; const int32_t* masks2;                                            // vipant_fbank_view_pair only: the second view
    int nsrc;                                                                      // vipant_fbank_mix(_src) only: rows of wave (>= the grid's b)
};

__global__ __launch_bounds__(256) void clip_mean_kernel(const float* __restrict__ wave, int64_t stride,
                                                        const int64_t* __restrict__ nsamples, float* __restrict__ mean) {
    __shared__ float red[256];
    const int clip = blockIdx.x;
    const int64_t n = nsamples[clip];
    const float* w = wave + (int64_t)clip * stride;
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += w[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[clip] = n > 0 ? red[0] / (float)n : 0.f;
}

// the partner of a clip: mix_index clamped into [-1, nsrc) -- the host cannot see a device array's values.  nsrc is the number of
// rows of wave, passed explicitly: the partner rows of vipant_fbank_mix_src lie past the b rows the grid covers.
__device__ __forceinline__ int mix_partner(const int32_t* __restrict__ mix_index, int clip, int nsrc) {
    const int p = mix_index[clip];
    return p < 0 ? -1 : (p >= nsrc ? nsrc - 1 : p);
}

// mixup on the waveform (cvap/data/audioset_cls.py:374-398): mean over nsamples[i] of x = lam c_i + (1 - lam) c_p, c = w - mean(w),
// the partner truncated or zero-padded to the clip's length.  One workgroup per clip; a clip is 640 KB at 10 s, so the pass is
// bound by how many loads one CU keeps in flight: 1024 threads, four independent strided partial sums each, then an LDS tree --
// a fixed order, no atomics.
constexpr int MIX_MEAN_THREADS = 1024;

__global__ __launch_bounds__(MIX_MEAN_THREADS) void mix_mean_kernel(const float* __restrict__ wave, int64_t stride,
                                                                    const int64_t* __restrict__ nsamples,
                                                                    const int32_t* __restrict__ mix_index,
                                                                    const float* __restrict__ mix_lambda,
                                                                    const float* __restrict__ mean, float* __restrict__ mix_mean,
                                                                    int nsrc) {
    constexpr int NT = MIX_MEAN_THREADS;
    __shared__ float red[NT];
    const int clip = blockIdx.x;
    const int p = mix_partner(mix_index, clip, nsrc);
    if (p < 0) {                                                  // uniform over the workgroup
        if (threadIdx.x == 0) mix_mean[clip] = 0.f;
        return;
    }
    const int64_t n = nsamples[clip];
    const int64_t np = nsamples[p] < stride ? nsamples[p] : stride;
    const float* w = wave + (int64_t)clip * stride;
    const float* wp = wave + (int64_t)p * stride;
    const float lam = mix_lambda[clip], oml = 1.f - lam, m = mean[clip], mp = mean[p];
    auto x = [&](int64_t i) { return lam * (w[i] - m) + oml * (i < np ? wp[i] - mp : 0.f); };
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int64_t i = threadIdx.x;
    for (; i + 3 * NT < n; i += 4 * NT) {
        s0 += x(i); s1 += x(i + NT); s2 += x(i + 2 * NT); s3 += x(i + 3 * NT);
    }
    for (; i < n; i += NT) s0 += x(i);
    red[threadIdx.x] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) mix_mean[clip] = n > 0 ? red[0] / (float)n : 0.f;
}

// ---- waveform views: the reference's waveform transforms and its crop rule (cvap/data/audio/transform.py:75-202, :24-28) ----------
// A clip passes through flip -> scale -> pad -> crop -> noise -> the pipeline's crop -> zero-mean.  None of the intermediate signals
// is stored: view_plan_kernel resolves every data-dependent decision of a clip (the crop rule compares standard deviations, the noise
// level follows the signal power) into a 64-byte plan, and view_sample() maps an output index back through the stages to one or two
// source samples.  Everything that needs the signal -- the plan's own reductions, the log-mel frame loader, wave_view_kernel --
// calls view_sample, so all of them see the same bits.
enum : int32_t { VIEW_FLIP = VIPANT_VIEW_FLIP, VIEW_SCALE = VIPANT_VIEW_SCALE, VIEW_PAD = VIPANT_VIEW_PAD, VIEW_CROP = VIPANT_VIEW_CROP,
                 VIEW_NOISE = VIPANT_VIEW_NOISE };
enum : int32_t { PLAN_FLIP = 1, PLAN_SCALED = 2, PLAN_NOISY = 4 };

struct ViewPlan {
    int32_t n0, n2, n3, n4, n_out;          // lengths: source (= after flip), after scale, after pad, after crop (what the noise sees), final
    int32_t flags;                          // PLAN_*
    int32_t pad_left, crop_left, final_left;
    float c, fill_l, fill_r, sigma, mean;   // scale factor, pad values, noise level, mean of the final window (0 without zero_mean)
    uint32_t key0, key1;                    // Philox key of the clip
};
static_assert(sizeof(ViewPlan) == 64, "plan layout");

// z(seed, clip, k): Philox4x32-10 with key (seed_lo, seed_hi ^ clip) and counter (k >> 2, 0, 0, 0); word k & 3 serves sample k, and
// Box-Muller runs over the word pairs (0, 1) and (2, 3) -- a function of k alone, because a sample is loaded by up to three
// overlapping frames and by the reductions and must have the same value every time.
__device__ __forceinline__ float view_normal(uint32_t k0, uint32_t k1, uint32_t k) {
    uint32_t c0 = k >> 2, c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const bool second = (k & 2u) != 0u;
    const uint32_t wu = second ? c2 : c0, wv = second ? c3 : c1;
    const float u = __fmul_rn((float)(wu >> 9) + 0.5f, 0x1p-23f), v = __fmul_rn((float)(wv >> 9) + 0.5f, 0x1p-23f);   // exact, in (0, 1)
    const float rad = sqrtf(__fmul_rn(-2.0f, logf(u)));
    return __fmul_rn(rad, (k & 1u) ? sinpif(__fmul_rn(2.0f, v)) : cospif(__fmul_rn(2.0f, v)));
}

// sample i of the scaled (and flipped) clip, 0 <= i < n2.  The blend is pinned (one product, one fused multiply-add) so that every
// kernel that inlines this rounds alike.
__device__ __forceinline__ float view_scaled(const ViewPlan& p, const float* __restrict__ w, int i) {
    const int last = p.n0 - 1;
    if (p.flags & PLAN_SCALED) {
        const float base = (float)i / p.c;                                    // IEEE fp32 division, as torch's arange().div_()
        int r1 = (int)base;
        r1 = r1 < last ? r1 : last;
        const int r2 = r1 + 1 < last ? r1 + 1 : last;
        const float r = base - (float)r1;
        const float a = w[(p.flags & PLAN_FLIP) ? last - r1 : r1], b = w[(p.flags & PLAN_FLIP) ? last - r2 : r2];
        return __fmaf_rn(r, b, __fmul_rn(1.0f - r, a));
    }
    i = i < last ? i : last;
    return w[(p.flags & PLAN_FLIP) ? last - i : i];
}

// sample j of the clip's final window, 0 <= j < n_out.  A plan whose later stages are not resolved yet (crop_left = final_left = 0,
// no noise, mean = 0) yields the signal in front of those stages: this is how view_plan_kernel's reductions use it.
__device__ __forceinline__ float view_sample(const ViewPlan& p, const float* __restrict__ w, int j) {
    const int k = j + p.final_left;                                           // index into the cropped signal: the noise counter
    const int i = k + p.crop_left - p.pad_left;                               // index into the scaled signal; outside it: padding
    float x = i < 0 ? p.fill_l : (i >= p.n2 ? p.fill_r : view_scaled(p, w, i));
    if (p.flags & PLAN_NOISY) x = __fmaf_rn(p.sigma, view_normal(p.key0, p.key1, (uint32_t)k), x);
    return x - p.mean;
}

constexpr int VIEW_PLAN_THREADS = 1024;

// sum of eight doubles per thread over the workgroup, in a fixed order: butterfly within a wave, the waves' sums through LDS, every
// thread then adds them in wave order (so all threads hold the same totals)
__device__ __forceinline__ void view_reduce8(double (&v)[8], double (*red)[8]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        double x = v[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) red[wv][q] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        double x = 0.0;
        for (int i = 0; i < VIEW_PLAN_THREADS / 64; ++i) x += red[i][q];
        v[q] = x;
    }
    __syncthreads();
}

__device__ __forceinline__ double view_var(double s, double q, int n) {      // unbiased, as torch.std
    const double v = (q - s * s / (double)n) / (double)(n - 1);
    return v > 0.0 ? v : 0.0;
}

__device__ __forceinline__ double view_unit(double u) { return u >= 0.0 ? (u < 1.0 ? u : 0x1.fffffffffffffp-1) : 0.0; }    // into [0, 1); NaN -> 0

// RandomCrop.random_crop (transform.py:122-141) of the signal view_sample(p, w, 0 .. n) to length len (< n): the drawn (or centred)
// window, unless its standard deviation is below half the clip's -- then the head, or the tail if the head is quieter still.
// Sums and sums of squares over the four windows (whole, drawn, head, tail) come from ONE pass, in double: these are variances of
// 10^5 samples that are then compared with each other.
__device__ __forceinline__ int view_crop_rule(const ViewPlan& p, const float* __restrict__ w, int n, int len, double u, bool center,
                                              double (*red)[8]) {
    const int d = n - len;
    int left;
    if (center) left = (d >> 1) + ((d & 1) ? ((d >> 1) & 1) : 0);            // int(round(0.5 * d)): half to even
    else {
        const double f = floor(view_unit(u) * (double)d);
        left = f < (double)(d - 1) ? (int)f : d - 1;                          // np.random.randint(0, d) never returns d
    }
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += VIEW_PLAN_THREADS) {
        const double x = (double)view_sample(p, w, i), xx = x * x;
        a[0] += x; a[1] += xx;
        if (i >= left && i < left + len) { a[2] += x; a[3] += xx; }
        if (i < len) { a[4] += x; a[5] += xx; }
        if (i >= d) { a[6] += x; a[7] += xx; }
    }
    view_reduce8(a, red);
    const double old_var = 0.25 * view_var(a[0], a[1], n), new_var = view_var(a[2], a[3], len);
    if (!(new_var < old_var)) return left;
    const double head_var = view_var(a[4], a[5], len);
    return new_var > head_var ? d : 0;
}

struct ViewParams { int32_t pad_len, crop_len, final_len, stages, train, zero_mean, has_padding_value; float padding_value; uint32_t seed_lo, seed_hi; };

__global__ __launch_bounds__(VIEW_PLAN_THREADS) void view_plan_kernel(const float* __restrict__ wave, int64_t stride,
                                                                      const int64_t* __restrict__ nsamples,
                                                                      const double* __restrict__ draws, ViewParams vp,
                                                                      ViewPlan* __restrict__ plans) {
    __shared__ double red[VIEW_PLAN_THREADS / 64][8];
    __shared__ float redf[256];
    const int clip = blockIdx.x;
    const float* w = wave + (int64_t)clip * stride;
    int64_t n0 = nsamples[clip];
    n0 = n0 < 0 ? 0 : (n0 < stride ? n0 : stride);
    ViewPlan p;
    p.n0 = p.n2 = p.n3 = p.n4 = p.n_out = (int)n0;
    p.flags = 0;
    p.pad_left = p.crop_left = p.final_left = 0;
    p.c = 1.f; p.fill_l = p.fill_r = p.sigma = p.mean = 0.f;
    p.key0 = vp.seed_lo; p.key1 = vp.seed_hi ^ (uint32_t)clip;
    if (n0 == 0) {                                                // uniform over the workgroup: an empty clip stays empty
        if (threadIdx.x == 0) plans[clip] = p;
        return;
    }
    const double* dr = draws + (int64_t)clip * 6;
    const double flip = dr[0], scale = dr[1], pad_u = dr[2], crop_u = dr[3], snr = dr[4], final_u = dr[5];
    if ((vp.stages & VIEW_FLIP) && flip >= 0.5) p.flags |= PLAN_FLIP;
    if ((vp.stages & VIEW_SCALE) && scale > 0.0 && scale != 1.0) {            // a factor that is not positive (or NaN) leaves the clip as it is
        double m = floor((double)p.n0 * scale);                               // int(n * scaling), the product in double
        m = m < 1.0 ? 1.0 : (m < 16777215.0 ? m : 16777215.0);                // fp32 indices are exact below 2^24
        p.n2 = (int)m; p.c = (float)scale; p.flags |= PLAN_SCALED;
    }
    p.n3 = p.n2;
    if ((vp.stages & VIEW_PAD) && p.n2 < vp.pad_len) {
        const int d = vp.pad_len - p.n2;
        const double f = floor(view_unit(pad_u) * (double)d);
        p.pad_left = f < (double)(d - 1) ? (int)f : d - 1;                    // np.random.randint(0, d) never returns d
        p.fill_l = vp.has_padding_value ? vp.padding_value : view_scaled(p, w, 0);
        p.fill_r = vp.has_padding_value ? vp.padding_value : view_scaled(p, w, p.n2 - 1);
        p.n3 = vp.pad_len;
    }
    p.n4 = p.n3;
    if ((vp.stages & VIEW_CROP) && p.n3 > vp.crop_len) {
        p.crop_left = view_crop_rule(p, w, p.n3, vp.crop_len, crop_u, false, red);
        p.n4 = vp.crop_len;
    }
    if ((vp.stages & VIEW_NOISE) && snr >= 0.0) {                             // RandomNoise.random_noise (transform.py:186-199)
        double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < p.n4; i += VIEW_PLAN_THREADS) {
            const double x = (double)view_sample(p, w, i);
            a[0] += x * x;
        }
        view_reduce8(a, red);
        const double power = a[0] / (double)p.n4;
        const float watts = (power > 0.0 ? (float)pow(10.0, (10.0 * log10(power) - snr) / 10.0) : 0.f) + 1e-7f;
        p.sigma = (float)sqrt((double)watts);
        p.flags |= PLAN_NOISY;
    }
    p.n_out = p.n4;
    if (p.n4 > vp.final_len) {
        p.final_left = view_crop_rule(p, w, p.n4, vp.final_len, final_u, !vp.train, red);
        p.n_out = vp.final_len;
    }
    if (vp.zero_mean) {                                           // clip_mean_kernel's order (256 strided partial sums, LDS tree), so that a
        float s = 0.f;                                            // clip with nothing to do gets vipant_fbank's mean to the bit
        if (threadIdx.x < 256)
            for (int i = threadIdx.x; i < p.n_out; i += 256) s += view_sample(p, w, i);
        if (threadIdx.x < 256) redf[threadIdx.x] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) redf[threadIdx.x] += redf[threadIdx.x + o];
            __syncthreads();
        }
        p.mean = redf[0] / (float)p.n_out;
    }
    if (threadIdx.x == 0) plans[clip] = p;
}

// the final waveform itself, for callers that want it (and for the tests): [b, out_stride], zero beyond a clip's n_out
__global__ __launch_bounds__(256) void wave_view_kernel(const float* __restrict__ wave, int64_t stride, const ViewPlan* __restrict__ plans,
                                                        float* __restrict__ out, int64_t out_stride, int64_t* __restrict__ nsamples_out,
                                                        int64_t b) {
    const int64_t total = b * out_stride, step = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += step) {
        const int64_t clip = e / out_stride, j = e - clip * out_stride;
        const ViewPlan p = plans[clip];
        const int64_t n = p.n_out < out_stride ? p.n_out : out_stride;
        out[e] = j < n ? view_sample(p, wave + clip * stride, (int)j) : 0.f;
        if (j == 0) nsamples_out[clip] = n;
    }
}

// LDS traffic of one wave is processed in program order, and a frame is private to its wave: between FFT passes it is
// enough to stop the compiler from moving LDS accesses across the pass boundary.
__device__ __forceinline__ void wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float2 cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

constexpr int FPW = 4;            // frame PAIRS per wave: the workgroup's tables (twiddles, window, mel weights) serve 32 frames
constexpr int MAXF = 256;         // mel bins

// MODE_MIX: a clip with a partner forms its samples from two sources on the way into LDS (the mixed waveform is never stored).
// MODE_VIEW: the clip's length comes from its plan and the samples from view_sample (the transformed waveform is never stored).
enum : int { MODE_PLAIN = 0, MODE_MIX = 1, MODE_VIEW = 2 };

// PAIR (MODE_VIEW only): two views of the same clips that differ in their masks alone (a.out / a.masks and a.out2 / a.masks2).  A
// frame pair whose two frames are live in the same way in both views is transformed once and stored twice.  Where the views
// disagree (a time-mask edge of one view inside the pair) each view that has a live frame gets a transform of its own, with
// exactly the frames it has live: a frame that is not live enters the packed transform as zeros, and its partner's rounding
// depends on that, so this is what keeps each view the bits of the single-view launch.
template <int NFFT, int MODE, bool PAIR>
__global__ __launch_bounds__(256) void fbank_kernel(FbankArgs a) {
    static_assert(!PAIR || MODE == MODE_VIEW, "the pair launch is a view launch");
    constexpr int NV = PAIR ? 2 : 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_off[MAXF + 1], s_start[MAXF], s_len[MAXF];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int clip = blockIdx.y;
    float2* tw = (float2*)smem;                                   // exp(-2 pi i k / NFFT), k < NFFT / 2
    float* win = (float*)(tw + NFFT / 2);                         // window, NFFT floats reserved
    float* wgt = win + NFFT;                                      // packed non-zero mel weights, <= NFFT floats
    float2* buf0 = (float2*)(wgt + NFFT) + (size_t)wave * 2 * NFFT;
    float2* buf1 = buf0 + NFFT;
    float* raw = (float*)buf1;                                    // the frame's samples before windowing

    // ---- workgroup tables
    for (int i = threadIdx.x; i < NFFT / 2; i += 256) {
        float sn, cs;
        sincospif(-2.0f * (float)i / (float)NFFT, &sn, &cs);      // exact at the power-of-two fractions
        tw[i] = make_float2(cs, sn);
    }
    for (int i = threadIdx.x; i < a.size; i += 256) win[i] = a.window[i];
    if ((int)threadIdx.x < a.F) { s_start[threadIdx.x] = a.bank_start[threadIdx.x]; s_len[threadIdx.x] = a.bank_len[threadIdx.x]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int o = 0;
        for (int m = 0; m < a.F; ++m) { s_off[m] = o; o += s_len[m]; }
        s_off[a.F] = o;
    }
    __syncthreads();
    const int nnz = s_off[a.F] <= NFFT ? s_off[a.F] : 0;          // more than two filters per bin: read the weights from global
    if (nnz > 0) {
        for (int m = wave; m < a.F; m += 4) {
            const float* row = a.banks + (int64_t)m * (NFFT / 2 + 1) + s_start[m];
            for (int k = lane; k < s_len[m]; k += 64) wgt[s_off[m] + k] = row[k];
        }
    }
    __syncthreads();

    ViewPlan plan;
    int64_t n;
    if constexpr (MODE == MODE_VIEW) {
        plan = a.plan[clip];
        n = plan.n_out;
    } else {
        n = a.nsamples[clip];
    }
    const int nframes = n < a.size ? 0 : (int)(1 + (n - a.size) / a.shift);
    const float cmean = a.clip_mean != nullptr ? a.clip_mean[clip] : 0.f;
    int vf0[NV], vf1[NV], vt0[NV], vt1[NV];
    float* vout[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int32_t* vm = v == 0 ? a.masks : a.masks2;
        const int32_t* mk = vm != nullptr ? vm + (int64_t)clip * 4 : nullptr;
        vf0[v] = vf1[v] = vt0[v] = vt1[v] = 0;
        if (mk != nullptr) { vf0[v] = mk[0]; vf1[v] = mk[1]; vt0[v] = mk[2]; vt1[v] = mk[3]; }
        vout[v] = v == 0 ? a.out : a.out2;
    }
    int partner = -1;
    int64_t np = 0;
    float lam = 1.f, oml = 0.f, pmean = 0.f, xmean = 0.f;
    if constexpr (MODE == MODE_MIX) {
        partner = mix_partner(a.mix_index, clip, a.nsrc);
        if (partner >= 0) {
            np = a.nsamples[partner] < a.wave_stride ? a.nsamples[partner] : a.wave_stride;
            lam = a.mix_lambda[clip]; oml = 1.f - lam;
            pmean = a.clip_mean[partner]; xmean = a.mix_mean[clip];
        }
    }

    // Two real frames share one complex transform: z = y_a + i y_b, and with Z = FFT(z)
    //   X_a[k] = (Z[k] + conj Z[N-k]) / 2,   X_b[k] = (Z[k] - conj Z[N-k]) / (2i)
    // so |X_a|^2 = ((Zr + Zr')^2 + (Zi - Zi')^2) / 4 and |X_b|^2 = ((Zi + Zi')^2 + (Zr' - Zr)^2) / 4 with Z' = Z[N-k].
    // A wave walks FPW frame pairs (2t, 2t + 1); the FFT's LDS traffic per frame halves.
    // (every decision below is uniform over the wave: ta depends on the wave, not on the lane)
#pragma unroll 1
    for (int step = 0; step < FPW * NV; ++step) {
        const int it = step / NV, vw = step % NV;                 // vw: the view whose live frames this transform serves
        const int ta = ((blockIdx.x * FPW + it) * 4 + wave) * 2, tb = ta + 1;
        if (ta >= a.T) break;
        const float padv = a.norm_std != 0.f ? (0.f - a.norm_mean) / a.norm_std : 0.f;
        bool vla[NV], vlb[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            vla[v] = ta < nframes && !(ta >= vt0[v] && ta < vt1[v]);
            vlb[v] = tb < a.T && tb < nframes && !(tb >= vt0[v] && tb < vt1[v]);
        }
        if (vw == 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int f0 = vf0[v], f1 = vf1[v], t0 = vt0[v], t1 = vt1[v];
                float* ra = vout[v] + ((int64_t)clip * a.T + ta) * a.F;
                float* rb = ra + a.F;
                if (!vla[v]) {                                    // padding row or time-masked row: constant
                    const bool tm = ta >= t0 && ta < t1;
                    for (int m = lane; m < a.F; m += 64) ra[m] = (tm || (m >= f0 && m < f1)) ? 0.f : padv;
                }
                if (!vlb[v] && tb < a.T) {
                    const bool tm = tb >= t0 && tb < t1;
                    for (int m = lane; m < a.F; m += 64) rb[m] = (tm || (m >= f0 && m < f1)) ? 0.f : padv;
                }
            }
        }
        bool both = false;                                        // this transform's rows go to the second view as well
        if constexpr (PAIR) {
            const bool same = vla[0] == vla[1] && vlb[0] == vlb[1];
            if (vw == 1 && same) continue;                        // served by the first view's transform
            both = vw == 0 && same;
        }
        const bool live_a = vla[vw], live_b = vlb[vw];
        const int f0 = vf0[vw], f1 = vf1[vw];
        float* dst_a = vout[vw] + ((int64_t)clip * a.T + ta) * a.F;
        float* dst_b = dst_a + a.F;
        if (!live_a && !live_b) continue;
        const float* src = a.wave + (int64_t)clip * a.wave_stride + (int64_t)ta * a.shift;
        const float* psrc = a.wave + (int64_t)(partner >= 0 ? partner : clip) * a.wave_stride;
        float* raw_b = raw + NFFT;
        float sa = 0.f, sb = 0.f;
        for (int j = lane; j < a.size; j += 64) {
            float xa, xb;
            if constexpr (MODE == MODE_VIEW) {
                const float* w = a.wave + (int64_t)clip * a.wave_stride;
                xa = live_a ? view_sample(plan, w, ta * a.shift + j) : 0.f;
                xb = live_b ? view_sample(plan, w, tb * a.shift + j) : 0.f;
            } else {
                xa = live_a ? src[j] - cmean : 0.f;
                xb = live_b ? src[j + a.shift] - cmean : 0.f;
            }
            if constexpr (MODE == MODE_MIX) {
                if (partner >= 0) {                               // the ORIGINAL partner clip, truncated / zero-padded to this clip
                    const int64_t ja = (int64_t)ta * a.shift + j, jb = ja + a.shift;
                    if (live_a) xa = (lam * xa + oml * (ja < np ? psrc[ja] - pmean : 0.f)) - xmean;
                    if (live_b) xb = (lam * xb + oml * (jb < np ? psrc[jb] - pmean : 0.f)) - xmean;
                }
            }
            raw[j] = xa; raw_b[j] = xb;
            sa += xa; sb += xb;
        }
        sa = wave_sum(sa); sb = wave_sum(sb);
        const float ma = sa / (float)a.size, mb = sb / (float)a.size;
        wave_lds_sync();
        for (int j = lane; j < NFFT; j += 64) {
            float ya = 0.f, yb = 0.f;
            if (j < a.size) {
                const int jp = j > 0 ? j - 1 : 0;
                const float w = win[j];
                ya = ((raw[j] - ma) - a.preemph * (raw[jp] - ma)) * w;
                yb = ((raw_b[j] - mb) - a.preemph * (raw_b[jp] - mb)) * w;
            }
            buf0[j] = make_float2(ya, yb);
        }
        wave_lds_sync();

        // Stockham autosort FFT: one radix-2 pass if log2(NFFT) is odd, then radix-4 passes (sub-transform length ns -> 4 ns)
        float2* in = buf0;
        float2* out = buf1;
        int ns = 1;
        if ((31 - __builtin_clz(NFFT)) & 1) {
            for (int j = lane; j < NFFT / 2; j += 64) {
                const float2 u = in[j], v = in[j + NFFT / 2];
                out[2 * j] = make_float2(u.x + v.x, u.y + v.y);
                out[2 * j + 1] = make_float2(u.x - v.x, u.y - v.y);
            }
            wave_lds_sync();
            float2* tmp = in; in = out; out = tmp;
            ns = 2;
        }
#pragma unroll 1
        for (; ns < NFFT; ns <<= 2) {
            const int tstep = NFFT / (4 * ns);
            for (int j = lane; j < NFFT / 4; j += 64) {
                const int k = j & (ns - 1);
                const int i1 = k * tstep;
                const float2 w1 = tw[i1], w2 = tw[2 * i1];
                float2 w3 = tw[(3 * i1) & (NFFT / 2 - 1)];
                if (3 * i1 >= NFFT / 2) w3 = make_float2(-w3.x, -w3.y);
                const float2 v0 = in[j], v1 = cmul(in[j + NFFT / 4], w1), v2 = cmul(in[j + NFFT / 2], w2),
                             v3 = cmul(in[j + 3 * NFFT / 4], w3);
                const float2 p = make_float2(v0.x + v2.x, v0.y + v2.y), q = make_float2(v0.x - v2.x, v0.y - v2.y);
                const float2 r = make_float2(v1.x + v3.x, v1.y + v3.y);
                const float2 d = make_float2(v1.y - v3.y, -(v1.x - v3.x));           // (v1 - v3) * (-i)
                const int o = ((j - k) << 2) + k;
                out[o] = make_float2(p.x + r.x, p.y + r.y);
                out[o + ns] = make_float2(q.x + d.x, q.y + d.y);
                out[o + 2 * ns] = make_float2(p.x - r.x, p.y - r.y);
                out[o + 3 * ns] = make_float2(q.x - d.x, q.y - d.y);
            }
            wave_lds_sync();
            float2* tmp = in; in = out; out = tmp;
        }
        // `in` holds Z; both frames' one-sided power spectra come from Z[k] and Z[N - k]
        for (int m = lane; m < a.F; m += 64) {
            const int k0 = s_start[m], len = s_len[m];
            const float* w = nnz > 0 ? wgt + s_off[m] : a.banks + (int64_t)m * (NFFT / 2 + 1) + k0;
            float ea = 0.f, eb = 0.f;
            for (int k = 0; k < len; ++k) {
                const float2 z = in[k0 + k], zc = in[(NFFT - (k0 + k)) & (NFFT - 1)];
                const float ar = z.x + zc.x, ai = z.y - zc.y, br = z.y + zc.y, bi = zc.x - z.x;
                const float wk = 0.25f * w[k];
                ea += (ar * ar + ai * ai) * wk;
                eb += (br * br + bi * bi) * wk;
            }
            const bool fm = m >= f0 && m < f1;
            bool fm2 = false;
            float* dst2_a = nullptr;
            if constexpr (PAIR) {
                fm2 = m >= vf0[1] && m < vf1[1];
                dst2_a = vout[1] + ((int64_t)clip * a.T + ta) * a.F;
            }
            if (live_a) {
                float v = logf(fmaxf(ea, 1.1920928955078125e-07f));
                if (a.norm_std != 0.f) v = (v - a.norm_mean) / a.norm_std;
                dst_a[m] = fm ? 0.f : v;
                if constexpr (PAIR) { if (both) dst2_a[m] = fm2 ? 0.f : v; }
            }
            if (live_b) {
                float v = logf(fmaxf(eb, 1.1920928955078125e-07f));
                if (a.norm_std != 0.f) v = (v - a.norm_mean) / a.norm_std;
                dst_b[m] = fm ? 0.f : v;
                if constexpr (PAIR) { if (both) dst2_a[a.F + m] = fm2 ? 0.f : v; }
            }
        }
        wave_lds_sync();                                          // the next pair overwrites both buffers
    }
}

template <int NFFT, int MODE, bool PAIR = false>
int32_t launch_fbank(const FbankArgs& a, int64_t b, hipStream_t s) {
    static DeviceOnce once;
    const size_t lds = ((size_t)4 * 2 * NFFT + NFFT / 2) * sizeof(float2) + (size_t)2 * NFFT * sizeof(float);
    if (first_on_device(once)) {
        VIPANT_HIP_TRY(hipFuncSetAttribute((const void*)fbank_kernel<NFFT, MODE, PAIR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        done_on_device(once);
    }
    hipLaunchKernelGGL((fbank_kernel<NFFT, MODE, PAIR>), dim3((unsigned)((a.T + 8 * FPW - 1) / (8 * FPW)), (unsigned)b), dim3(256), lds, s, a);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

}  // namespace

extern "C" size_t vipant_fbank_workspace_bytes(int64_t b) { return (size_t)((b * 4 + 255) / 256 * 256); }

extern "C" int32_t vipant_fbank(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                                const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                                int64_t b, int64_t T, int64_t F, int32_t window_size, int32_t window_shift, int32_t nfft,
                                float preemphasis, int32_t zero_mean, float norm_mean, float norm_std, void* workspace,
                                size_t workspace_bytes, void* stream) {
    VIPANT_REQUIRE(b > 0 && b < 65536 && T > 0 && F > 0 && F <= 256, VIPANT_EBADSHAPE, "fbank: bad batch b=%ld T=%ld F=%ld", (long)b, (long)T, (long)F);
    VIPANT_REQUIRE(nfft == 512 || nfft == 1024 || nfft == 2048, VIPANT_EBADSHAPE, "fbank: padded window %d not in {512, 1024, 2048}", nfft);
    VIPANT_REQUIRE(window_size > 1 && window_size <= nfft && window_size > nfft / 2 && window_shift > 0, VIPANT_EBADSHAPE,
                   "fbank: bad window %d / shift %d for padded size %d", window_size, window_shift, nfft);
    VIPANT_REQUIRE(wave != nullptr && nsamples != nullptr && out != nullptr && window != nullptr && banks != nullptr &&
                       bank_start != nullptr && bank_len != nullptr, VIPANT_EBADSHAPE, "fbank: null argument");
    VIPANT_REQUIRE(!zero_mean || (workspace != nullptr && workspace_bytes >= vipant_fbank_workspace_bytes(b)), VIPANT_ENOWORKSPACE,
                   "fbank: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    float* cmean = nullptr;
    if (zero_mean) {
        cmean = (float*)workspace;
        hipLaunchKernelGGL(clip_mean_kernel, dim3((unsigned)b), dim3(256), 0, s, wave, wave_stride, nsamples, cmean);
        VIPANT_LAUNCH_CHECK();
    }
    FbankArgs a{wave, wave_stride, nsamples, out, window, banks, bank_start, bank_len, masks, cmean, nullptr, nullptr, nullptr,
                (int)T, (int)F, window_size, window_shift, preemphasis, norm_mean, norm_std};
    switch (nfft) {
        case 512: return launch_fbank<512, MODE_PLAIN>(a, b, s);
        case 1024: return launch_fbank<1024, MODE_PLAIN>(a, b, s);
        default: return launch_fbank<2048, MODE_PLAIN>(a, b, s);
    }
}

namespace {

// vipant_fbank_mix is the nsrc == b case: the same three launches with the same grids over the b output rows, so it keeps its bits
int32_t fbank_mix_impl(const char* who, const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                       const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                       const int32_t* mix_index, const float* mix_lambda, int64_t nsrc, int64_t b, int64_t T, int64_t F,
                       int32_t window_size, int32_t window_shift, int32_t nfft, float preemphasis, float norm_mean, float norm_std,
                       void* workspace, size_t workspace_bytes, size_t workspace_need, void* stream) {
    VIPANT_REQUIRE(b > 0 && b < 65536 && T > 0 && F > 0 && F <= 256, VIPANT_EBADSHAPE, "%s: bad batch b=%ld T=%ld F=%ld", who, (long)b, (long)T, (long)F);
    VIPANT_REQUIRE(nsrc >= b && nsrc < 65536, VIPANT_EBADSHAPE, "%s: %ld source rows for b=%ld", who, (long)nsrc, (long)b);
    VIPANT_REQUIRE(nfft == 512 || nfft == 1024 || nfft == 2048, VIPANT_EBADSHAPE, "%s: padded window %d not in {512, 1024, 2048}", who, nfft);
    VIPANT_REQUIRE(window_size > 1 && window_size <= nfft && window_size > nfft / 2 && window_shift > 0, VIPANT_EBADSHAPE,
                   "%s: bad window %d / shift %d for padded size %d", who, window_size, window_shift, nfft);
    VIPANT_REQUIRE(wave != nullptr && nsamples != nullptr && out != nullptr && window != nullptr && banks != nullptr &&
                       bank_start != nullptr && bank_len != nullptr && mix_index != nullptr && mix_lambda != nullptr,
                   VIPANT_EBADSHAPE, "%s: null argument", who);
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= workspace_need, VIPANT_ENOWORKSPACE, "%s: workspace too small", who);
    hipStream_t s = (hipStream_t)stream;
    float* cmean = (float*)workspace;                             // nsrc means, then the b means of the mixed clips
    float* xmean = cmean + nsrc;
    hipLaunchKernelGGL(clip_mean_kernel, dim3((unsigned)nsrc), dim3(256), 0, s, wave, wave_stride, nsamples, cmean);
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(mix_mean_kernel, dim3((unsigned)b), dim3(MIX_MEAN_THREADS), 0, s, wave, wave_stride, nsamples, mix_index, mix_lambda, cmean, xmean,
                       (int)nsrc);
    VIPANT_LAUNCH_CHECK();
    FbankArgs a{wave, wave_stride, nsamples, out, window, banks, bank_start, bank_len, masks, cmean, mix_index, mix_lambda, xmean,
                (int)T, (int)F, window_size, window_shift, preemphasis, norm_mean, norm_std, nullptr, nullptr, (int)nsrc};
    switch (nfft) {
        case 512: return launch_fbank<512, MODE_MIX>(a, b, s);
        case 1024: return launch_fbank<1024, MODE_MIX>(a, b, s);
        default: return launch_fbank<2048, MODE_MIX>(a, b, s);
    }
}

}  // namespace

// per-clip means only: mean(w_i) and the mean of the mixed clip, b floats each
extern "C" size_t vipant_fbank_mix_workspace_bytes(int64_t b) { return (size_t)((b * 8 + 255) / 256 * 256); }

extern "C" int32_t vipant_fbank_mix(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                                    const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                                    const int32_t* mix_index, const float* mix_lambda, int64_t b, int64_t T, int64_t F,
                                    int32_t window_size, int32_t window_shift, int32_t nfft, float preemphasis, float norm_mean,
                                    float norm_std, void* workspace, size_t workspace_bytes, void* stream) {
    return fbank_mix_impl("fbank_mix", wave, wave_stride, nsamples, out, window, banks, bank_start, bank_len, masks, mix_index, mix_lambda,
                          b, b, T, F, window_size, window_shift, nfft, preemphasis, norm_mean, norm_std, workspace, workspace_bytes,
                          b > 0 ? vipant_fbank_mix_workspace_bytes(b) : 0, stream);
}

// mean(w_r) of all nsrc rows and the mean of the b mixed clips
extern "C" size_t vipant_fbank_mix_src_workspace_bytes(int64_t nsrc, int64_t b) { return (size_t)(((nsrc + b) * 4 + 255) / 256 * 256); }

extern "C" int32_t vipant_fbank_mix_src(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                                        const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                                        const int32_t* mix_index, const float* mix_lambda, int64_t nsrc, int64_t b, int64_t T,
                                        int64_t F, int32_t window_size, int32_t window_shift, int32_t nfft, float preemphasis,
                                        float norm_mean, float norm_std, void* workspace, size_t workspace_bytes, void* stream) {
    VIPANT_REQUIRE(wave_stride >= 1, VIPANT_EBADSHAPE, "fbank_mix_src: bad stride %ld", (long)wave_stride);
    return fbank_mix_impl("fbank_mix_src", wave, wave_stride, nsamples, out, window, banks, bank_start, bank_len, masks, mix_index,
                          mix_lambda, nsrc, b, T, F, window_size, window_shift, nfft, preemphasis, norm_mean, norm_std, workspace,
                          workspace_bytes, b > 0 && nsrc >= b ? vipant_fbank_mix_src_workspace_bytes(nsrc, b) : 0, stream);
}

// one 64-byte plan per clip
extern "C" size_t vipant_fbank_view_workspace_bytes(int64_t b) { return (size_t)((b * (int64_t)sizeof(ViewPlan) + 255) / 256 * 256); }

namespace {

// the checks the two view entry points share, and the plan launch; nothing is launched unless everything holds
int32_t launch_view_plan(const char* who, const float* wave, int64_t wave_stride, const int64_t* nsamples, int64_t b,
                         const vipant_view_params& vp, const double* draws, void* workspace, size_t workspace_bytes, hipStream_t s) {
    VIPANT_REQUIRE(b > 0 && b < 65536 && wave_stride > 0 && wave_stride < (int64_t)1 << 31, VIPANT_EBADSHAPE, "%s: bad batch b=%ld stride=%ld", who,
                   (long)b, (long)wave_stride);
    VIPANT_REQUIRE(wave != nullptr && nsamples != nullptr && draws != nullptr, VIPANT_EBADSHAPE, "%s: null argument", who);
    const int64_t lim = (int64_t)1 << 30;
    VIPANT_REQUIRE(vp.final_len >= 2 && vp.final_len < lim, VIPANT_EBADSHAPE, "%s: final length %ld outside [2, 2^30)", who, (long)vp.final_len);
    VIPANT_REQUIRE(!(vp.stages & VIEW_PAD) || (vp.pad_len >= 1 && vp.pad_len < lim), VIPANT_EBADSHAPE, "%s: pad length %ld outside [1, 2^30)", who,
                   (long)vp.pad_len);
    VIPANT_REQUIRE(!(vp.stages & VIEW_CROP) || (vp.crop_len >= 2 && vp.crop_len < lim), VIPANT_EBADSHAPE, "%s: crop length %ld outside [2, 2^30)", who,
                   (long)vp.crop_len);
    VIPANT_REQUIRE((vp.stages & ~31) == 0, VIPANT_EBADSHAPE, "%s: unknown stage bits 0x%x", who, (unsigned)vp.stages);
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= vipant_fbank_view_workspace_bytes(b), VIPANT_ENOWORKSPACE, "%s: workspace too small", who);
    const ViewParams k{(int32_t)vp.pad_len, (int32_t)vp.crop_len, (int32_t)vp.final_len, vp.stages, vp.train, vp.zero_mean,
                       vp.has_padding_value, vp.padding_value, (uint32_t)(vp.seed & 0xFFFFFFFFu), (uint32_t)(vp.seed >> 32)};
    hipLaunchKernelGGL(view_plan_kernel, dim3((unsigned)b), dim3(VIEW_PLAN_THREADS), 0, s, wave, wave_stride, nsamples, draws, k, (ViewPlan*)workspace);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

}  // namespace

namespace {

// vipant_fbank_view and vipant_fbank_view_pair: `who` names the entry point in messages, pair selects the two-view kernel
int32_t fbank_view_common(const char* who, bool pair, const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out,
                          float* out2, const float* window, const float* banks, const int32_t* bank_start, const int32_t* bank_len,
                          const int32_t* masks, const int32_t* masks2, int64_t b, int64_t T, int64_t F, int32_t window_size,
                          int32_t window_shift, int32_t nfft, float preemphasis, float norm_mean, float norm_std,
                          const vipant_view_params& view, const double* draws, void* workspace, size_t workspace_bytes, void* stream) {
    VIPANT_REQUIRE(b > 0 && b < 65536 && T > 0 && F > 0 && F <= 256, VIPANT_EBADSHAPE, "%s: bad batch b=%ld T=%ld F=%ld", who, (long)b, (long)T, (long)F);
    VIPANT_REQUIRE(nfft == 512 || nfft == 1024 || nfft == 2048, VIPANT_EBADSHAPE, "%s: padded window %d not in {512, 1024, 2048}", who, nfft);
    VIPANT_REQUIRE(window_size > 1 && window_size <= nfft && window_size > nfft / 2 && window_shift > 0, VIPANT_EBADSHAPE,
                   "%s: bad window %d / shift %d for padded size %d", who, window_size, window_shift, nfft);
    VIPANT_REQUIRE(out != nullptr && window != nullptr && banks != nullptr && bank_start != nullptr && bank_len != nullptr, VIPANT_EBADSHAPE,
                   "%s: null argument", who);
    if (pair) {
        VIPANT_REQUIRE(out2 != nullptr, VIPANT_EBADSHAPE, "%s: null second output", who);
        const uintptr_t lo = (uintptr_t)out, lo2 = (uintptr_t)out2, bytes = (uintptr_t)(b * T * F) * sizeof(float);
        VIPANT_REQUIRE(lo + bytes <= lo2 || lo2 + bytes <= lo, VIPANT_EBADSHAPE, "%s: the two outputs overlap", who);
    }
    hipStream_t s = (hipStream_t)stream;
    const int32_t rc = launch_view_plan(who, wave, wave_stride, nsamples, b, view, draws, workspace, workspace_bytes, s);
    if (rc != VIPANT_OK) return rc;
    FbankArgs a{wave, wave_stride, nsamples, out, window, banks, bank_start, bank_len, masks, nullptr, {nullptr}, nullptr, nullptr,
                (int)T, (int)F, window_size, window_shift, preemphasis, norm_mean, norm_std, out2, masks2};
    a.plan = (const ViewPlan*)workspace;
    if (pair) {
        switch (nfft) {
            case 512: return launch_fbank<512, MODE_VIEW, true>(a, b, s);
            case 1024: return launch_fbank<1024, MODE_VIEW, true>(a, b, s);
            default: return launch_fbank<2048, MODE_VIEW, true>(a, b, s);
        }
    }
    switch (nfft) {
        case 512: return launch_fbank<512, MODE_VIEW>(a, b, s);
        case 1024: return launch_fbank<1024, MODE_VIEW>(a, b, s);
        default: return launch_fbank<2048, MODE_VIEW>(a, b, s);
    }
}

}  // namespace

extern "C" int32_t vipant_fbank_view(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, const float* window,
                                     const float* banks, const int32_t* bank_start, const int32_t* bank_len, const int32_t* masks,
                                     int64_t b, int64_t T, int64_t F, int32_t window_size, int32_t window_shift, int32_t nfft,
                                     float preemphasis, float norm_mean, float norm_std, vipant_view_params view, const double* draws,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return fbank_view_common("fbank_view", false, wave, wave_stride, nsamples, out, nullptr, window, banks, bank_start, bank_len, masks,
                             nullptr, b, T, F, window_size, window_shift, nfft, preemphasis, norm_mean, norm_std, view, draws, workspace,
                             workspace_bytes, stream);
}

extern "C" int32_t vipant_fbank_view_pair(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* out, float* out2,
                                          const float* window, const float* banks, const int32_t* bank_start, const int32_t* bank_len,
                                          const int32_t* masks, const int32_t* masks2, int64_t b, int64_t T, int64_t F,
                                          int32_t window_size, int32_t window_shift, int32_t nfft, float preemphasis, float norm_mean,
                                          float norm_std, vipant_view_params view, const double* draws, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    return fbank_view_common("fbank_view_pair", true, wave, wave_stride, nsamples, out, out2, window, banks, bank_start, bank_len, masks,
                             masks2, b, T, F, window_size, window_shift, nfft, preemphasis, norm_mean, norm_std, view, draws, workspace,
                             workspace_bytes, stream);
}

extern "C" int32_t vipant_wave_view(const float* wave, int64_t wave_stride, const int64_t* nsamples, float* wave_out, int64_t out_stride,
                                    int64_t* nsamples_out, int64_t b, vipant_view_params view, const double* draws, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    VIPANT_REQUIRE(wave_out != nullptr && nsamples_out != nullptr && out_stride > 0 && out_stride < (int64_t)1 << 31, VIPANT_EBADSHAPE,
                   "wave_view: bad output (stride %ld)", (long)out_stride);
    hipStream_t s = (hipStream_t)stream;
    const int32_t rc = launch_view_plan("wave_view", wave, wave_stride, nsamples, b, view, draws, workspace, workspace_bytes, s);
    if (rc != VIPANT_OK) return rc;
    const int64_t blocks = ceil_div(b * out_stride, 256);
    hipLaunchKernelGGL(wave_view_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, wave, wave_stride,
                       (const ViewPlan*)workspace, wave_out, out_stride, nsamples_out, b);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}
