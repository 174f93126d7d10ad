// PCM ingest (gfx950, wave64): a ragged batch of 16-bit interleaved PCM clips [b, pcm_stride] in, the fp32 mono waveforms
// [b, wave_stride] the log-mel front-end takes out, in one launch.  It is what the reference's loader processes do per file between
// the decoder and the filter bank: torchaudio.load(normalize=True) -- int16 * 2^-15 -- and the head of _extract_kaldi_spectrogram
// (cvap/data/audio/transform.py:15-21): the channel rule and `tile_audio`.
//   VIPANT_PCM_FIRST  w[j] = pcm[j ch] * 2^-15: channel 0, which is what kaldi.fbank takes of a multi-channel waveform (image_audio.py
//                     leaves mean_channel off)
//   VIPANT_PCM_MEAN   w[j] = (float(sum_c pcm[j ch + c]) * 2^-15) / float(ch): the sum in int32 (exact), the product exact, ONE IEEE
//                     division -- the bits of torch's (x.float() / 32768).mean(0) on the CPU (a multiply by 1 / ch is not: ch = 3, 5, 6, 7)
//   tile_len > 0      a clip of 0 < n < tile_len frames is repeated to n * ceil(tile_len / n) samples (the reference's slice after
//                     torch.tile cuts the channel axis, so nothing is truncated: that length is kept), clamped to wave_stride
// nframes / channels are DEVICE arrays (the host never waits on them), so they are clamped here, not refused: channels into [1, 8]
// before any use, nframes into [0, pcm_stride / channels] -- no read leaves a clip's row of pcm.  Every element of [b, wave_stride]
// is written exactly once (zero beyond a clip's length), nothing else is; nsamples_out[i] = the length, at most wave_stride.
// A thread forms 8 consecutive samples: the mono and stereo cases load them as one or two 16-byte words when the unit lies inside the
// clip without wrapping and its address is 16-byte aligned, everything else goes sample by sample; the stores are two 16-byte words
// under the same condition on the output.  No workspace, no atomics, no LDS: the same input gives the same bits.
#include "common.h"

namespace {

constexpr int PCM_UNIT = 8, PCM_THREADS = 256, PCM_MAX_CH = 8;
constexpr float PCM_SCALE = 1.0f / 32768.0f;
typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float pcm_mono(const int16_t* __restrict__ p, int ch, int mode) {
    if (mode == VIPANT_PCM_FIRST || ch == 1) return (float)p[0] * PCM_SCALE;
    int32_t sum = 0;
    for (int c = 0; c < ch; ++c) sum += p[c];
    return __fdiv_rn((float)sum * PCM_SCALE, (float)ch);
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_wave_kernel(const int16_t* __restrict__ pcm, int64_t pcm_stride,
                                                                const int64_t* __restrict__ nframes, const int32_t* __restrict__ channels,
                                                                int mode, int64_t tile_len, float* __restrict__ wave, int64_t wave_stride,
                                                                int64_t* __restrict__ nsamples_out, int64_t b) {
    const int64_t units = (wave_stride + PCM_UNIT - 1) / PCM_UNIT, total = b * units, step = (int64_t)gridDim.x * PCM_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * PCM_THREADS + threadIdx.x; e < total; e += step) {
        const int64_t clip = e / units, j0 = (e - clip * units) * PCM_UNIT;
        int ch = channels[clip];
        ch = ch < 1 ? 1 : (ch > PCM_MAX_CH ? PCM_MAX_CH : ch);
        const int64_t nmax = pcm_stride / ch;
        int64_t n = nframes[clip];
        n = n < 0 ? 0 : (n > nmax ? nmax : n);
        const bool tiled = tile_len > 0 && n > 0 && n < tile_len;
        int64_t nout = tiled ? n * ((tile_len + n - 1) / n) : n;
        nout = nout < wave_stride ? nout : wave_stride;
        if (j0 == 0) nsamples_out[clip] = nout;
        const int cnt = (int)(wave_stride - j0 < PCM_UNIT ? wave_stride - j0 : PCM_UNIT);      // samples of this unit inside the row
        const int64_t s0 = tiled ? j0 % n : j0;                                                // source frame of the unit's first sample
        const int16_t* src = pcm + clip * pcm_stride + s0 * ch;
        float v[PCM_UNIT];
        if (j0 + PCM_UNIT <= nout && s0 + PCM_UNIT <= n && ch <= 2 && ((uintptr_t)src & 15) == 0) {
            const s16x8 q0 = *(const s16x8*)src;                       // frames s0 .. s0 + 7 lie inside [0, n): within the clip's row
            if (ch == 1) {
#pragma unroll
                for (int k = 0; k < PCM_UNIT; ++k) v[k] = (float)q0[k] * PCM_SCALE;
            } else {
                const s16x8 q1 = *(const s16x8*)(src + 8);
#pragma unroll
                for (int k = 0; k < PCM_UNIT; ++k) {
                    const int l = k < 4 ? q0[2 * k] : q1[2 * k - 8], r = k < 4 ? q0[2 * k + 1] : q1[2 * k - 7];
                    v[k] = mode == VIPANT_PCM_FIRST ? (float)l * PCM_SCALE : __fdiv_rn((float)(l + r) * PCM_SCALE, 2.0f);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < PCM_UNIT; ++k) {
                const int64_t j = j0 + k;
                float x = 0.f;
                if (j < nout) {                                        // (nout > 0 implies n > 0; the frame index is below n)
                    const int64_t f = tiled ? (s0 + k) % n : j;
                    x = pcm_mono(pcm + clip * pcm_stride + f * ch, ch, mode);
                }
                v[k] = x;
            }
        }
        float* dst = wave + clip * wave_stride + j0;
        if (cnt == PCM_UNIT && ((uintptr_t)dst & 15) == 0) {
            *(f32x4*)dst = f32x4{v[0], v[1], v[2], v[3]};
            *(f32x4*)(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
#pragma unroll
            for (int k = 0; k < PCM_UNIT; ++k)
                if (k < cnt) dst[k] = v[k];
        }
    }
}

}  // namespace

extern "C" int32_t vipant_pcm_wave(const int16_t* pcm, int64_t pcm_stride, const int64_t* nframes, const int32_t* channels, int32_t mode,
                                   int64_t tile_len, float* wave, int64_t wave_stride, int64_t* nsamples_out, int64_t b, void* stream) {
    constexpr int64_t LIM = (int64_t)1 << 40;
    VIPANT_REQUIRE(pcm && nframes && channels && wave && nsamples_out, VIPANT_EBADSHAPE, "pcm_wave: NULL argument");
    VIPANT_REQUIRE(b >= 1 && b < ((int64_t)1 << 20), VIPANT_EBADSHAPE, "pcm_wave: b = %lld outside [1, 2^20)", (long long)b);
    VIPANT_REQUIRE(pcm_stride >= 1 && pcm_stride < LIM && wave_stride >= 1 && wave_stride < LIM, VIPANT_EBADSHAPE,
                   "pcm_wave: strides (%lld, %lld) outside [1, 2^40)", (long long)pcm_stride, (long long)wave_stride);
    VIPANT_REQUIRE(mode == VIPANT_PCM_FIRST || mode == VIPANT_PCM_MEAN, VIPANT_EBADSHAPE, "pcm_wave: unknown mode %d", (int)mode);
    VIPANT_REQUIRE(tile_len >= 0 && tile_len < LIM, VIPANT_EBADSHAPE, "pcm_wave: tile_len = %lld outside [0, 2^40)", (long long)tile_len);
    const int64_t blocks = ceil_div(b * ceil_div(wave_stride, PCM_UNIT), PCM_THREADS);
    hipLaunchKernelGGL(pcm_wave_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(PCM_THREADS), 0, (hipStream_t)stream, pcm,
                       pcm_stride, nframes, channels, (int)mode, tile_len, wave, wave_stride, nsamples_out, b);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}
