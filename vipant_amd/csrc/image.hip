// The image towers' input stage (gfx950, wave64): decoded uint8 frames [b, Hmax, Wmax, 3] in, normalised fp32 [b, 3, n, n] out.
// Replaces what the reference does per frame in loader processes, in PIL: make_clip_image_transform (Resize(bicubic) + CenterCrop +
// ToTensor + Normalize, cvap/data/image/transform.py:11-18) and BarlowImageTransform (RandomResizedCrop(bicubic), flip, ColorJitter,
// grayscale, Gaussian blur, solarisation, Normalize, transform.py:146-200).  Three kernels:
//   image_plan_kernel      one workgroup per image: the draw row (or the Resize + CenterCrop rule) -> a 32-word plan and the two
//                          coefficient tables of PIL's bicubic resample (xmin, count, int32 coefficients per output index), in fp64
//                          with individually rounded operations, so that their bits are those of PIL's precompute_coeffs;
//   image_resample_kernel  one workgroup per (image, band of IMG_BAND output rows): the horizontal pass over the source rows the band
//                          needs goes to LDS as uint8 (PIL's intermediate), the vertical pass reads LDS; integer multiply-accumulate,
//                          the flip folded into the column index.  An image without a photometric stage is normalised here: the
//                          `clip` chain is this launch plus the plan, and no uint8 image ever exists in HBM;
//   image_photo_kernel     one workgroup per image, in place on its fp32 [3, n, n] code values, stages in plan order; pointwise stages
//                          are collected and applied in one pass, the contrast mean is an integer sum (exact, so the same bits on
//                          every run), the six box passes of the blur alternate between the image and one scratch plane.
// The limit on the downscale: a source extent (frame side for `clip`, crop box side otherwise) of at most IMG_MAX_SCALE = 8 times the
// resized extent, per axis, and n <= IMG_MAX_N = 224: at most 33 coefficients per output index and 90 source rows per band (60 KB LDS).
#include <math.h>

#include "common.h"

namespace {

constexpr int IMG_MAX_N = 224, IMG_MAX_SCALE = 8, IMG_KMAX = 33, IMG_KSTRIDE = 36, IMG_BAND = 8;
constexpr int IMG_MAX_ROWS = (IMG_BAND - 1) * IMG_MAX_SCALE + 1 + IMG_KMAX;           // 90
constexpr int IMG_TILE_BYTES = IMG_MAX_ROWS * IMG_MAX_N * 3;                          // 60480
constexpr int IMG_THREADS = 256, IMG_PLAN_WORDS = 32, IMG_DRAW = 16, IMG_MAX_OPS = 8;
constexpr int IMG_PHOTO = VIPANT_IMAGE_JITTER | VIPANT_IMAGE_GRAY | VIPANT_IMAGE_BLUR | VIPANT_IMAGE_SOLARISE;

// plan words: int32 unless noted
enum { P_Y0, P_X0, P_INH, P_INW, P_OUTH, P_OUTW, P_OFFY, P_OFFX, P_FLIP, P_PHOTO, P_ORD0, P_ORD1, P_ORD2, P_ORD3, P_GRAY, P_SOLAR,
       P_BLUR_L /* -1 = no blur */, P_FAC0 /* fp32 x 4 */, P_BLUR_A = P_FAC0 + 4 /* fp32 */, P_BLUR_DEN /* fp32 */ };
// draw columns (fp64): box top, left, height, width; flip; the order of the four jitter operations (-1 = no jitter); their factors
// (brightness, contrast, saturation, hue); gray; sigma (0 = no blur); solarise
enum { D_Y0, D_X0, D_H, D_W, D_FLIP, D_ORD0, D_FAC0 = D_ORD0 + 4, D_GRAY = D_FAC0 + 4, D_SIGMA, D_SOLAR };
enum { OP_BRIGHT, OP_CONTRAST, OP_SAT, OP_HUE, OP_GRAY, OP_SOLAR, OP_NORM };

struct ImgNorm { float mean[3], std[3]; };

struct Layout { size_t hw, draws, plan, tabs, scratch, total; };
inline Layout layout(int64_t b, int64_t n) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    Layout l;
    l.hw = 0;
    l.draws = up(l.hw + (size_t)b * 2 * sizeof(int32_t));
    l.plan = up(l.draws + (size_t)b * IMG_DRAW * sizeof(double));
    l.tabs = up(l.plan + (size_t)b * IMG_PLAN_WORDS * sizeof(int32_t));
    l.scratch = up(l.tabs + (size_t)b * 2 * n * IMG_KSTRIDE * sizeof(int32_t));
    l.total = up(l.scratch + (size_t)b * n * n * sizeof(float));
    return l;
}

// Python's int(round(d / 2.0)) for d >= 0: half to even
__host__ __device__ inline int half_even(int d) { return (d >> 1) + ((d & 1) & (d >> 1)); }

// Resize(n): the shorter side to n, the longer to int(n * long / short)
__host__ __device__ inline void resize_hw(int H, int W, int n, int* oh, int* ow) {
    if (W <= H) {
        *ow = n;
        *oh = (int)((double)((int64_t)n * H) / (double)W);
    } else {
        *oh = n;
        *ow = (int)((double)((int64_t)n * W) / (double)H);
    }
}

__device__ inline double bicubic(double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
    return 0.0;
}

// one entry of a coefficient table, as PIL's precompute_coeffs + normalize_coeffs_8bpc: output index `i` of a resize of `in` to `out`
__device__ inline void table_entry(int32_t* e, int i, int in, int out) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    const double center = ((double)i + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    int cnt = xmax - xmin;
    cnt = cnt < 0 ? 0 : (cnt > IMG_KMAX ? IMG_KMAX : cnt);
    double ww = 0.0;
    for (int k = 0; k < cnt; ++k) ww += bicubic(((double)(k + xmin) - center + 0.5) * ss);
    e[0] = xmin;
    e[1] = cnt;
    for (int k = 0; k < cnt; ++k) {
        double w = bicubic(((double)(k + xmin) - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        e[2 + k] = w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
    }
}

__global__ __launch_bounds__(IMG_THREADS) void image_plan_kernel(const int32_t* __restrict__ hw, const double* __restrict__ draws,
                                                                  int32_t* __restrict__ plans, int32_t* __restrict__ tabs, int n,
                                                                  int chain) {
    __shared__ int32_t s_plan[IMG_PLAN_WORDS];
    const int img = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        const int H = hw[2 * img], W = hw[2 * img + 1];
        for (int k = 0; k < IMG_PLAN_WORDS; ++k) s_plan[k] = 0;
        float* pf = (float*)s_plan;
        s_plan[P_ORD0] = -1;
        s_plan[P_BLUR_L] = -1;
        if (!draws) {
            int oh, ow;
            resize_hw(H, W, n, &oh, &ow);
            s_plan[P_INH] = H, s_plan[P_INW] = W, s_plan[P_OUTH] = oh, s_plan[P_OUTW] = ow;
            s_plan[P_OFFY] = half_even(oh - n), s_plan[P_OFFX] = half_even(ow - n);
        } else {
            const double* d = draws + (int64_t)img * IMG_DRAW;
            s_plan[P_Y0] = (int)d[D_Y0], s_plan[P_X0] = (int)d[D_X0], s_plan[P_INH] = (int)d[D_H], s_plan[P_INW] = (int)d[D_W];
            s_plan[P_OUTH] = s_plan[P_OUTW] = n;
            s_plan[P_FLIP] = (chain & VIPANT_IMAGE_FLIP) && d[D_FLIP] != 0.0;
            int photo = 0;
            if ((chain & VIPANT_IMAGE_JITTER) && d[D_ORD0] >= 0.0) {
                photo = 1;
                for (int q = 0; q < 4; ++q) {
                    const int op = (int)d[D_ORD0 + q];
                    s_plan[P_ORD0 + q] = op < 0 ? 0 : (op > 3 ? 3 : op);
                    pf[P_FAC0 + q] = (float)d[D_FAC0 + q];
                }
            }
            if ((chain & VIPANT_IMAGE_GRAY) && d[D_GRAY] != 0.0) s_plan[P_GRAY] = photo = 1;
            if ((chain & VIPANT_IMAGE_SOLARISE) && d[D_SOLAR] != 0.0) s_plan[P_SOLAR] = photo = 1;
            if ((chain & VIPANT_IMAGE_BLUR) && d[D_SIGMA] > 0.0) {          // PIL's GaussianBlur: three extended box passes per axis
                const double s2 = d[D_SIGMA] * d[D_SIGMA] / 3.0;
                const double L = sqrt(12.0 * s2 + 1.0);
                const double l = floor((L - 1.0) / 2.0);
                const double a = (2.0 * l + 1.0) * (l * (l + 1.0) - 3.0 * s2) / (6.0 * (s2 - (l + 1.0) * (l + 1.0)));
                s_plan[P_BLUR_L] = (int)l;
                pf[P_BLUR_A] = (float)a;
                pf[P_BLUR_DEN] = (float)(2.0 * (l + a) + 1.0);
                photo = 1;
            }
            s_plan[P_PHOTO] = photo;
        }
    }
    __syncthreads();
    if (tid < IMG_PLAN_WORDS) plans[(int64_t)img * IMG_PLAN_WORDS + tid] = s_plan[tid];
    int32_t* tab = tabs + (int64_t)img * 2 * n * IMG_KSTRIDE;            // [axis: 0 = columns, 1 = rows][n][IMG_KSTRIDE]
    for (int e = tid; e < 2 * n; e += IMG_THREADS) {
        const int axis = e / n, i = e - axis * n;
        if (axis == 0) table_entry(tab + (int64_t)e * IMG_KSTRIDE, i + s_plan[P_OFFX], s_plan[P_INW], s_plan[P_OUTW]);
        else table_entry(tab + (int64_t)e * IMG_KSTRIDE, i + s_plan[P_OFFY], s_plan[P_INH], s_plan[P_OUTH]);
    }
}

__device__ __forceinline__ int clip8(int acc) {
    acc >>= 22;
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// ToTensor + Normalize: three individually rounded fp32 operations
__device__ __forceinline__ float normalise(float v, float mean, float std) {
    return __fdiv_rn(__fsub_rn(__fdiv_rn(v, 255.0f), mean), std);
}

__global__ __launch_bounds__(IMG_THREADS) void image_resample_kernel(const uint8_t* __restrict__ frames, int64_t sb, int64_t sh,
                                                                      int64_t sw, const int32_t* __restrict__ plans,
                                                                      const int32_t* __restrict__ tabs, float* __restrict__ out, int n,
                                                                      ImgNorm norm) {
    __shared__ uint8_t tile[IMG_TILE_BYTES];                            // [source row of the band][channel][column]
    const int img = blockIdx.y, tid = threadIdx.x;
    const int r0 = blockIdx.x * IMG_BAND, r1 = min(r0 + IMG_BAND, n), nb = r1 - r0;
    const int32_t* pl = plans + (int64_t)img * IMG_PLAN_WORDS;
    const int32_t* tx = tabs + (int64_t)img * 2 * n * IMG_KSTRIDE;
    const int32_t* ty = tx + (int64_t)n * IMG_KSTRIDE;
    const int y0 = pl[P_Y0], x0 = pl[P_X0], inh = pl[P_INH], inw = pl[P_INW], flip = pl[P_FLIP], photo = pl[P_PHOTO];
    const int ybase = ty[r0 * IMG_KSTRIDE];
    int rows = ty[(r1 - 1) * IMG_KSTRIDE] + ty[(r1 - 1) * IMG_KSTRIDE + 1] - ybase;
    rows = min(min(rows, IMG_MAX_ROWS), inh - ybase);                   // (both hold by construction: the host checked the limit)
    const uint8_t* src0 = frames + (int64_t)img * sb + (int64_t)(y0 + ybase) * sh + (int64_t)x0 * sw;
    for (int idx = tid; idx < rows * 3 * n; idx += IMG_THREADS) {
        const int j = idx % n, rc = idx / n, c = rc % 3, r = rc / 3;
        const int32_t* e = tx + (flip ? n - 1 - j : j) * IMG_KSTRIDE;
        const int xmin = e[0], cnt = min(min(e[1], IMG_KMAX), inw - xmin);
        const uint8_t* src = src0 + (int64_t)r * sh + (int64_t)xmin * sw + c;
        int acc = 1 << 21;
        for (int k = 0; k < cnt; ++k) acc += e[2 + k] * (int)src[(int64_t)k * sw];
        tile[rc * n + j] = (uint8_t)clip8(acc);
    }
    __syncthreads();
    for (int idx = tid; idx < nb * 3 * n; idx += IMG_THREADS) {
        const int j = idx % n, ic = idx / n, i = r0 + ic % nb, c = ic / nb;
        const int32_t* e = ty + i * IMG_KSTRIDE;
        const int ymin = e[0] - ybase, cnt = min(min(e[1], IMG_KMAX), rows - ymin);
        int acc = 1 << 21;
        for (int k = 0; k < cnt; ++k) acc += e[2 + k] * (int)tile[((ymin + k) * 3 + c) * n + j];
        const float v = (float)clip8(acc);
        const float m = c == 0 ? norm.mean[0] : (c == 1 ? norm.mean[1] : norm.mean[2]);
        const float s = c == 0 ? norm.std[0] : (c == 1 ? norm.std[1] : norm.std[2]);
        out[(((int64_t)img * 3 + c) * n + i) * n + j] = photo ? v : normalise(v, m, s);
    }
}

// PIL's convert("L") on code values: floor((19595 r + 38470 g + 7471 b) / 65536 + 0.5); exact in fp32 for integer r, g, b
__device__ __forceinline__ float luma(float r, float g, float b) {
#pragma clang fp contract(off)
    return floorf((19595.0f * r + 38470.0f * g + 7471.0f * b) / 65536.0f + 0.5f);
}
__device__ __forceinline__ float blend(float deg, float alpha, float x) {
    const float v = deg + alpha * (x - deg);
    return fminf(fmaxf(v, 0.0f), 255.0f);
}
// Python's colorsys.rgb_to_hsv, h = frac(h + shift), colorsys.hsv_to_rgb, on code values
__device__ inline void hue_shift(float& r, float& g, float& b, float shift) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    if (minc == maxc) return;
    const float range = maxc - minc, s = range / maxc, v = maxc;
    const float rc = (maxc - r) / range, gc = (maxc - g) / range, bc = (maxc - b) / range;
    float h = r == maxc ? bc - gc : (g == maxc ? 2.0f + rc - bc : 4.0f + gc - rc);
    h = h / 6.0f;
    h = h - floorf(h);
    h = h + shift;
    h = h - floorf(h);
    const float h6 = h * 6.0f;
    int i = (int)h6;
    const float f = h6 - (float)i;
    const float p = v * (1.0f - s), q = v * (1.0f - s * f), t = v * (1.0f - s * (1.0f - f));
    i = i % 6;
    switch (i) {
        case 0: r = v, g = t, b = p; break;
        case 1: r = q, g = v, b = p; break;
        case 2: r = p, g = v, b = t; break;
        case 3: r = p, g = q, b = v; break;
        case 4: r = t, g = p, b = v; break;
        default: r = v, g = p, b = q; break;
    }
}

__device__ inline void apply_ops(float& r, float& g, float& b, const int* ops, const float* pa, const float* pb, int nops,
                                 const ImgNorm& norm) {
    for (int q = 0; q < nops; ++q) {
        const float a = pa[q];
        switch (ops[q]) {
            case OP_BRIGHT: r = blend(0.0f, a, r), g = blend(0.0f, a, g), b = blend(0.0f, a, b); break;
            case OP_CONTRAST: r = blend(pb[q], a, r), g = blend(pb[q], a, g), b = blend(pb[q], a, b); break;
            case OP_SAT: {
                const float l = luma(r, g, b);
                r = blend(l, a, r), g = blend(l, a, g), b = blend(l, a, b);
                break;
            }
            case OP_HUE: hue_shift(r, g, b, a); break;
            case OP_GRAY: r = g = b = luma(r, g, b); break;
            case OP_SOLAR:
                r = r >= 128.0f ? 255.0f - r : r, g = g >= 128.0f ? 255.0f - g : g, b = b >= 128.0f ? 255.0f - b : b;
                break;
            default:
                r = normalise(r, norm.mean[0], norm.std[0]), g = normalise(g, norm.mean[1], norm.std[1]);
                b = normalise(b, norm.mean[2], norm.std[2]);
                break;
        }
    }
}

// one extended box pass along `step` (1 = a row, n = a column): inner taps -l .. l, the two outer taps weighted a, clamp to the edge
__device__ inline void box_pass(const float* __restrict__ src, float* __restrict__ dst, int n, bool vertical, int l, float a, float den,
                                int tid) {
    for (int p = tid; p < n * n; p += IMG_THREADS) {
        const int y = p / n, x = p - y * n;
        const int pos = vertical ? y : x, base = vertical ? x : y * n, step = vertical ? n : 1;
        float acc = 0.0f;
        for (int d = -l; d <= l; ++d) acc += src[base + min(max(pos + d, 0), n - 1) * step];
        const float outer = src[base + max(pos - l - 1, 0) * step] + src[base + min(pos + l + 1, n - 1) * step];
        dst[p] = (acc + a * outer) / den;
    }
}

__global__ __launch_bounds__(IMG_THREADS) void image_photo_kernel(float* __restrict__ out, const int32_t* __restrict__ plans,
                                                                   float* __restrict__ scratch, int n, ImgNorm norm) {
    __shared__ int s_ops[IMG_MAX_OPS];
    __shared__ float s_pa[IMG_MAX_OPS], s_pb[IMG_MAX_OPS];
    __shared__ int s_sum[IMG_THREADS / WAVE];
    const int img = blockIdx.x, tid = threadIdx.x, np = n * n;
    const int32_t* pl = plans + (int64_t)img * IMG_PLAN_WORDS;
    const float* pf = (const float*)pl;
    if (!pl[P_PHOTO]) return;                                           // the resample launch has written the final values
    float* im = out + (int64_t)img * 3 * np;
    float* scr = scratch + (int64_t)img * np;
    int nops = 0;                                                       // (every thread keeps the same count; the lists are in LDS)
    if (pl[P_ORD0] >= 0) {
        for (int q = 0; q < 4; ++q) {
            const int op = pl[P_ORD0 + q];
            const float fac = pf[P_FAC0 + op];
            if (op == OP_HUE ? fac == 0.0f : fac == 1.0f) continue;     // a neutral factor leaves the image as it is, bit for bit
            float deg = 0.0f;
            if (op == OP_CONTRAST) {                                    // the mean of L over the image as it is at this point
                __syncthreads();                                        // (the pending operations are visible)
                int sum = 0;
                for (int p = tid; p < np; p += IMG_THREADS) {
                    float r = im[p], g = im[np + p], b = im[2 * np + p];
                    apply_ops(r, g, b, s_ops, s_pa, s_pb, nops, norm);
                    sum += (int)luma(r, g, b);
                }
                for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
                if ((tid & 63) == 0) s_sum[tid >> 6] = sum;
                __syncthreads();
                int total = 0;
                for (int w = 0; w < IMG_THREADS / WAVE; ++w) total += s_sum[w];
                deg = (float)floor((double)total / (double)np + 0.5);
            }
            if (tid == 0) s_ops[nops] = op, s_pa[nops] = fac, s_pb[nops] = deg;
            ++nops;
        }
    }
    if (pl[P_GRAY]) {
        if (tid == 0) s_ops[nops] = OP_GRAY, s_pa[nops] = 0.0f, s_pb[nops] = 0.0f;
        ++nops;
    }
    if (pl[P_BLUR_L] >= 0) {
        __syncthreads();
        for (int p = tid; p < np; p += IMG_THREADS) {
            float r = im[p], g = im[np + p], b = im[2 * np + p];
            apply_ops(r, g, b, s_ops, s_pa, s_pb, nops, norm);
            im[p] = r, im[np + p] = g, im[2 * np + p] = b;
        }
        nops = 0;
        const int l = pl[P_BLUR_L];
        const float a = pf[P_BLUR_A], den = pf[P_BLUR_DEN];
        for (int c = 0; c < 3; ++c) {
            float* plane = im + (int64_t)c * np;
            for (int pass = 0; pass < 6; ++pass) {                      // three along the rows, three along the columns
                __syncthreads();
                box_pass(pass & 1 ? scr : plane, pass & 1 ? plane : scr, n, pass >= 3, l, a, den, tid);
            }
        }
        __syncthreads();
    }
    if (pl[P_SOLAR]) {
        if (tid == 0) s_ops[nops] = OP_SOLAR, s_pa[nops] = 0.0f, s_pb[nops] = 0.0f;
        ++nops;
    }
    if (tid == 0) s_ops[nops] = OP_NORM, s_pa[nops] = 0.0f, s_pb[nops] = 0.0f;
    ++nops;
    __syncthreads();
    for (int p = tid; p < np; p += IMG_THREADS) {
        float r = im[p], g = im[np + p], b = im[2 * np + p];
        apply_ops(r, g, b, s_ops, s_pa, s_pb, nops, norm);
        im[p] = r, im[np + p] = g, im[2 * np + p] = b;
    }
}

}  // namespace

extern "C" size_t vipant_image_view_workspace_bytes(int64_t b, int64_t n, int64_t max_h, int64_t max_w) {
    if (b < 1 || n < 1 || n > IMG_MAX_N || max_h < 1 || max_w < 1) return 0;
    return layout(b, n).total;
}

extern "C" int32_t vipant_image_view(const uint8_t* frames, int64_t stride_b, int64_t stride_h, int64_t stride_w, int64_t max_h,
                                     int64_t max_w, const int32_t* hw, const double* draws, vipant_image_params params, float* out,
                                     int64_t b, void* workspace, size_t workspace_bytes, void* stream) {
    const int n = params.n;
    VIPANT_REQUIRE(frames && hw && out && workspace, VIPANT_EBADSHAPE, "image_view: NULL argument");
    VIPANT_REQUIRE(b >= 1 && b <= 65535, VIPANT_EBADSHAPE, "image_view: b = %lld outside [1, 65535]", (long long)b);
    VIPANT_REQUIRE(n >= 1 && n <= IMG_MAX_N, VIPANT_EBADSHAPE, "image_view: n = %d outside [1, %d]", n, IMG_MAX_N);
    VIPANT_REQUIRE(max_h >= 1 && max_w >= 1 && max_h < (1 << 24) && max_w < (1 << 24) && stride_w >= 3 && stride_h >= max_w * stride_w &&
                       stride_b >= max_h * stride_h,
                   VIPANT_EBADSHAPE, "image_view: frames [%lld, %lld, %lld, 3] with strides (%lld, %lld, %lld, 1) overlap or are empty",
                   (long long)b, (long long)max_h, (long long)max_w, (long long)stride_b, (long long)stride_h, (long long)stride_w);
    for (int c = 0; c < 3; ++c)
        VIPANT_REQUIRE(params.std[c] != 0.0f, VIPANT_EBADSHAPE, "image_view: std[%d] = 0", c);
    const Layout lay = layout(b, n);
    VIPANT_REQUIRE(workspace_bytes >= lay.total, VIPANT_ENOWORKSPACE, "image_view: workspace of %zu bytes, %zu needed", workspace_bytes,
                   lay.total);
    for (int64_t i = 0; i < b; ++i) {                                   // every refusal happens here, before anything is written
        const int H = hw[2 * i], W = hw[2 * i + 1];
        VIPANT_REQUIRE(H >= 1 && W >= 1 && H <= max_h && W <= max_w, VIPANT_EBADSHAPE,
                       "image_view: frame %lld is %d x %d, outside [1, %lld] x [1, %lld]", (long long)i, H, W, (long long)max_h,
                       (long long)max_w);
        if (!draws) {
            int oh, ow;
            resize_hw(H, W, n, &oh, &ow);
            VIPANT_REQUIRE(H <= (int64_t)IMG_MAX_SCALE * oh && W <= (int64_t)IMG_MAX_SCALE * ow, VIPANT_EBADSHAPE,
                           "image_view: frame %lld (%d x %d) to %d x %d is beyond the downscale limit of %d per axis", (long long)i, H, W,
                           oh, ow, IMG_MAX_SCALE);
        } else {
            const double* d = draws + i * IMG_DRAW;
            bool ok = true;
            for (int k = 0; k < 4; ++k) ok = ok && d[k] >= 0.0 && d[k] < 16777216.0 && d[k] == floor(d[k]);
            VIPANT_REQUIRE(ok && d[D_H] >= 1.0 && d[D_W] >= 1.0 && d[D_Y0] + d[D_H] <= H && d[D_X0] + d[D_W] <= W, VIPANT_EBADSHAPE,
                           "image_view: box (%g, %g, %g, %g) of frame %lld is not an integer box inside %d x %d", d[D_Y0], d[D_X0],
                           d[D_H], d[D_W], (long long)i, H, W);
            VIPANT_REQUIRE(d[D_H] <= (double)IMG_MAX_SCALE * n && d[D_W] <= (double)IMG_MAX_SCALE * n, VIPANT_EBADSHAPE,
                           "image_view: box %g x %g of frame %lld to %d x %d is beyond the downscale limit of %d per axis", d[D_H],
                           d[D_W], (long long)i, n, n, IMG_MAX_SCALE);
            if ((params.chain & VIPANT_IMAGE_JITTER) && d[D_ORD0] >= 0.0) {
                int seen = 0;
                for (int q = 0; q < 4; ++q) {
                    const double o = d[D_ORD0 + q];
                    if (o == 0.0 || o == 1.0 || o == 2.0 || o == 3.0) seen |= 1 << (int)o;
                }
                VIPANT_REQUIRE(seen == 15, VIPANT_EBADSHAPE, "image_view: the jitter order of frame %lld is no permutation of 0..3",
                               (long long)i);
            }
            VIPANT_REQUIRE(d[D_SIGMA] >= 0.0 && d[D_SIGMA] < 1e3, VIPANT_EBADSHAPE, "image_view: sigma %g of frame %lld", d[D_SIGMA],
                           (long long)i);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int32_t* d_hw = (int32_t*)(ws + lay.hw);
    double* d_draws = draws ? (double*)(ws + lay.draws) : nullptr;
    int32_t* plans = (int32_t*)(ws + lay.plan);
    int32_t* tabs = (int32_t*)(ws + lay.tabs);
    VIPANT_HIP_TRY(hipMemcpyAsync(d_hw, hw, (size_t)b * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (draws) VIPANT_HIP_TRY(hipMemcpyAsync(d_draws, draws, (size_t)b * IMG_DRAW * sizeof(double), hipMemcpyHostToDevice, s));
    ImgNorm norm;
    for (int c = 0; c < 3; ++c) norm.mean[c] = params.mean[c], norm.std[c] = params.std[c];
    image_plan_kernel<<<dim3((unsigned)b), dim3(IMG_THREADS), 0, s>>>(d_hw, d_draws, plans, tabs, n, params.chain);
    VIPANT_LAUNCH_CHECK();
    image_resample_kernel<<<dim3((unsigned)ceil_div(n, IMG_BAND), (unsigned)b), dim3(IMG_THREADS), 0, s>>>(
        frames, stride_b, stride_h, stride_w, plans, tabs, out, n, norm);
    VIPANT_LAUNCH_CHECK();
    if (draws && (params.chain & IMG_PHOTO)) {
        image_photo_kernel<<<dim3((unsigned)b), dim3(IMG_THREADS), 0, s>>>(out, plans, (float*)(ws + lay.scratch), n, norm);
        VIPANT_LAUNCH_CHECK();
    }
    return VIPANT_OK;
}
