"""GPU log-mel front-end: the step in front of the hot path.

The reference computes one Kaldi filter bank per clip on CPU dataloader workers
(cvap/data/audio/transform.py:12-35, parameters cvap/data/image_audio.py:119-126), pads / normalises it and applies
SpecAugment masks (image_audio.py:183-207, configs/running/audio/default.yaml).  `KaldiFbank` does the same for a whole
batch of device-resident waveforms in two launches (`vipant_fbank`; three with waveform mixup, `vipant_fbank_mix`) and returns the [b, 1, T, F] tensor
`ViTPreEncoder` takes.  With `outputs=b` the mixup partners may be rows of `wave` past the b clips of the batch (`vipant_fbank_mix_src`):
the file loader draws a partner from the whole dataset and ships its clip behind the batch; such a row is read, never written.  File decoding stays with the loader (vipant_amd/data); `pcm_wave` turns the 16-bit PCM it decodes into
those waveforms in one launch (`vipant_pcm_wave`: int16 -> fp32, the channel rule, `tile_audio`).  On this path there is no resampling:
a dataset has one rate.

Under `running.audio.native_pcm` the loader ships the samples as the files hold them and every clip keeps its own sample rate, as in
the reference (torchaudio.load normalises any width, kaldi.fbank is called with the file's rate): `pcm_ingest` converts 8 / 16 / 24 /
32-bit PCM and 32-bit float on the device (`vipant_pcm_ingest`), and `RateFbank` groups a batch by rate and runs one
`vipant_fbank_rows` call per rate class over a list of rows, at padded sizes 256 .. 8192.  With
`running.audio.resample_to` the clips are brought to that one rate first, on the device (`Resample`: `vipant_resample`, the windowed
sinc of torchaudio.functional.resample), and the filter bank is the `KaldiFbank` of that rate.
The two filter banks share a base, `Fbank`: the settings read from `running.audio` (`fbank_config`), the host draws, the argument
rules of `__call__` and the view plan; each says its `crop_len_for(rate)`.  `clip_waves` is the one ingest door of the trainers, for a
PcmBatch and a RawPcmBatch alike; the host's copy of the lengths comes from `pcm_lengths` / `raw_lengths`.  What the trainers make of
all this per batch -- which draws, in which order -- is stated in vipant_amd/audio_batch.py.

What the reference does to the waveform in front of the filter bank (transform.py:22-28) happens inside the launch as well
(`vipant_fbank_view`): the `running.audio.audio_transforms` chain of transform.py:75-202 -- any subsequence of RandomFlip,
RandomScale, RandomPad, RandomCrop, RandomNoise in that order -- when `transform_audio` is on and the loader is training, and
always the crop to int((max_len / 100 + 0.05) * sample_rate) samples with its standard-deviation rule.  The random draws are made
on the host (`draw_views`), one reduction launch turns them into a per-clip plan, and the frame loader forms each sample from
the original clip: the transformed waveform is never stored (`view_wave` materialises it for whoever wants to look at it).

The siamese dataset wants two SpecAugment views of one log-mel (FbankTransform, transform.py:223-258): `pair=True` writes both from
one filter-bank launch (`vipant_fbank_view_pair`), each with the bits of the single call under its masks.

The filter tables (Hann window, mel weights) are built once per (sample rate, bins) with torch ops on the device.
SpecAugment start / width draws follow torchaudio.functional.mask_along_axis (two uniform draws per mask, CPU generator),
one (frequency, time) pair per clip as the reference's per-item transform does.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import ops
from . import _ffi
from ._ffi import VipantError, call, query
from .data import RawPcmBatch

F32 = torch.float32


def _tables(sample_rate: float, num_mel_bins: int, frame_shift_ms: float, frame_length_ms: float, device):
    shift = int(sample_rate * frame_shift_ms * 0.001)
    size = int(sample_rate * frame_length_ms * 0.001)
    padded = 1 << (size - 1).bit_length()
    window = torch.hann_window(size, periodic=False, dtype=F32, device=device)
    nyquist = 0.5 * sample_rate
    mel = lambda f: 1127.0 * math.log(1.0 + f / 700.0)
    mel_lo, mel_hi = mel(20.0), mel(nyquist)
    delta = (mel_hi - mel_lo) / (num_mel_bins + 1)
    b = torch.arange(num_mel_bins, dtype=F32, device=device).unsqueeze(1)
    left, center, right = mel_lo + b * delta, mel_lo + (b + 1.0) * delta, mel_lo + (b + 2.0) * delta
    freqs = (sample_rate / padded) * torch.arange(padded // 2, dtype=F32, device=device)
    melf = (1127.0 * torch.log(1.0 + freqs / 700.0)).unsqueeze(0)
    banks = torch.clamp_min(torch.minimum((melf - left) / (center - left), (right - melf) / (right - center)), 0.0)
    banks = torch.nn.functional.pad(banks, (0, 1)).contiguous()
    nz = banks > 0
    start = nz.int().argmax(dim=1).to(torch.int32)
    length = nz.sum(dim=1).to(torch.int32)
    return shift, size, padded, window, banks, start.contiguous(), length.contiguous()


CHAIN = ("RandomFlip", "RandomScale", "RandomPad", "RandomCrop", "RandomNoise")
# the constructor signatures of transform.py:75-202: (name, default) in positional order
_SIGNATURES = {
    "RandomFlip": (("p", 0.5),),
    "RandomScale": (("scale", 1.5), ("keep_len", False)),
    "RandomPad": (("output_len", 88200), ("train", True), ("padding_value", None)),
    "RandomCrop": (("output_len", 44100), ("train", True)),
    "RandomNoise": (("snr_min_db", 10.0), ("snr_max_db", 120.0), ("p", 0.25)),
}


def _chain_error(why: str) -> VipantError:
    return VipantError(f"running.audio.audio_transforms: {why}; the accepted chain is any subsequence of "
                       f"{', '.join(CHAIN)}, in that order (RandomScale without keep_len, RandomPad / RandomCrop with train=True)")


def parse_audio_transforms(transforms) -> dict:
    """`running.audio.audio_transforms` -> {transform name: {parameter: value}}.  Entries are (name, params) with params a
    mapping (keywords) or a sequence (positional), as the reference's make_transform takes them (transform.py:41-45)."""
    chain, last = {}, -1
    for entry in transforms or ():
        try:
            name, params = entry
        except (TypeError, ValueError):
            raise _chain_error(f"entry {entry!r} is not a (name, parameters) pair") from None
        name = str(name)
        if name not in CHAIN:
            raise _chain_error(f"`{name}' is not supported")
        if name in chain:
            raise _chain_error(f"`{name}' appears twice")
        if CHAIN.index(name) < last:
            raise _chain_error(f"`{name}' is out of order")
        last = CHAIN.index(name)
        sig = _SIGNATURES[name]
        args = {k: v for k, v in sig}
        if hasattr(params, "keys"):
            for k in params.keys():
                if k not in args:
                    raise _chain_error(f"`{name}' has no parameter `{k}'")
                args[k] = params[k]
        else:
            params = list(params if params is not None else ())
            if len(params) > len(sig):
                raise _chain_error(f"`{name}' takes at most {len(sig)} parameters, got {len(params)}")
            for (k, _), v in zip(sig, params):
                args[k] = v
        if name == "RandomScale" and args["keep_len"]:
            raise _chain_error("RandomScale(keep_len=True) is not supported")
        if name in ("RandomPad", "RandomCrop") and not args["train"]:
            raise _chain_error(f"{name}(train=False) is not supported")
        chain[name] = args
    return chain


PCM_MODES = {"first": _ffi.PCM_FIRST, "mean": _ffi.PCM_MEAN}
PCM_MAX_CHANNELS = 8


def pcm_wave(pcm: torch.Tensor, nframes: torch.Tensor, channels: torch.Tensor, mode: str = "first", tile_len: int = 0,
             wave_stride: Optional[int] = None):
    """Decoded 16-bit PCM -> the waveforms `KaldiFbank.__call__(wave, nsamples, ...)` takes, in one launch (`vipant_pcm_wave`):
    what torchaudio.load(normalize=True) and the head of _extract_kaldi_spectrogram (transform.py:15-21) do per file.
    pcm int16 [b, stride] on the device, clip i = nframes[i] frames of channels[i] interleaved samples (int64 / int32 [b]; they are
    moved to the device, and nobody waits for them).  mode `first`: channel 0 (what kaldi.fbank takes); `mean`: the channel mean,
    with torch's CPU bits.  tile_len > 0: a clip shorter than tile_len is repeated to n * ceil(tile_len / n) samples
    (`running.audio.tile_audio`).  wave_stride: the width of the result (a longer clip is cut to it); default: the longest clip
    `stride` can hold, or twice tile_len where tiling can exceed that.  -> (wave fp32 [b, wave_stride], zero beyond a clip's length;
    nsamples int64 [b])."""
    if not isinstance(pcm, torch.Tensor) or not pcm.is_cuda:
        raise VipantError("pcm_wave: pcm must be a device tensor (there is no CPU path)")
    if pcm.dtype != torch.int16 or pcm.dim() != 2:
        raise VipantError(f"pcm_wave: pcm must be a 2-d int16 tensor, got {pcm.dtype} {tuple(pcm.shape)}")
    if mode not in PCM_MODES:
        raise VipantError(f"pcm_wave: mode `{mode}' is not one of {', '.join(PCM_MODES)}")
    pcm = pcm.contiguous()
    b, stride = pcm.shape
    dev = pcm.device
    nframes = torch.as_tensor(nframes).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
    channels = torch.as_tensor(channels).to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    if nframes.shape != (b,) or channels.shape != (b,):
        raise VipantError(f"pcm_wave: nframes / channels must have shape [{b}], got {tuple(nframes.shape)} / {tuple(channels.shape)}")
    tile_len = int(tile_len)
    if wave_stride is None:
        wave_stride = max(int(stride), 1)
        if 0 < tile_len and stride < 2 * tile_len:          # a tiled clip has fewer than 2 tile_len samples
            wave_stride = max(2 * tile_len - 2, wave_stride)
    wave = torch.empty((b, int(wave_stride)), dtype=F32, device=dev)
    nsamples = torch.empty((b,), dtype=torch.int64, device=dev)
    call("vipant_pcm_wave", pcm.data_ptr(), stride, nframes.data_ptr(), channels.data_ptr(), PCM_MODES[mode], tile_len,
         wave.data_ptr(), int(wave_stride), nsamples.data_ptr(), b, ops._stream())
    return wave, nsamples


def pcm_ingest(raw: torch.Tensor, nframes: torch.Tensor, channels: torch.Tensor, fmt: torch.Tensor, mode: str = "first",
               tile_len: Optional[torch.Tensor] = None, wave_stride: Optional[int] = None):
    """`pcm_wave` for the samples as a WAV file ships them (`vipant_pcm_ingest`): raw uint8 [b, byte_stride] on the device, clip i =
    nframes[i] frames of channels[i] interleaved little-endian samples of format fmt[i] (_ffi.PCM_U8 / S16 / S24 / S32 / F32), with
    the values of torchaudio.load(normalize=True).  tile_len int64 [b] or None: each clip's own tile length (the reference tiles to
    int(max_len / 100 * rate) at the file's rate); it is moved to the device like the other arrays.  wave_stride: the width of the
    result (default: the most frames a row can hold, 8-bit mono).  -> (wave fp32 [b, wave_stride], nsamples int64 [b])."""
    if not isinstance(raw, torch.Tensor) or not raw.is_cuda:
        raise VipantError("pcm_ingest: raw must be a device tensor (there is no CPU path)")
    if raw.dtype != torch.uint8 or raw.dim() != 2:
        raise VipantError(f"pcm_ingest: raw must be a 2-d uint8 tensor, got {raw.dtype} {tuple(raw.shape)}")
    if mode not in PCM_MODES:
        raise VipantError(f"pcm_ingest: mode `{mode}' is not one of {', '.join(PCM_MODES)}")
    raw = raw.contiguous()
    b, stride = raw.shape
    dev = raw.device
    nframes = torch.as_tensor(nframes).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
    channels = torch.as_tensor(channels).to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    fmt = torch.as_tensor(fmt).to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    if nframes.shape != (b,) or channels.shape != (b,) or fmt.shape != (b,):
        raise VipantError(f"pcm_ingest: nframes / channels / fmt must have shape [{b}], got {tuple(nframes.shape)} / "
                          f"{tuple(channels.shape)} / {tuple(fmt.shape)}")
    if tile_len is not None:
        tile_len = torch.as_tensor(tile_len).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
        if tile_len.shape != (b,):
            raise VipantError(f"pcm_ingest: tile_len must have shape [{b}], got {tuple(tile_len.shape)}")
    if wave_stride is None:
        wave_stride = max(int(stride), 1)
    wave = torch.empty((b, int(wave_stride)), dtype=F32, device=dev)
    nsamples = torch.empty((b,), dtype=torch.int64, device=dev)
    call("vipant_pcm_ingest", raw.data_ptr(), stride, nframes.data_ptr(), channels.data_ptr(), fmt.data_ptr(), PCM_MODES[mode],
         tile_len.data_ptr() if tile_len is not None else None, wave.data_ptr(), int(wave_stride), nsamples.data_ptr(), b, ops._stream())
    return wave, nsamples


def _tiled(n, tile_len):
    """The lengths after `tile_audio`: a clip shorter than tile_len is repeated to n * ceil(tile_len / n) samples."""
    return torch.where((n > 0) & (n < tile_len), n * ((tile_len + n - 1) // n.clamp(min=1)), n)


def pcm_lengths(nframes, channels, stride: int, tile_len: int = 0):
    """The lengths `pcm_wave` will report, from the host's copies of a PcmBatch's arrays (no device sync) -> n int64 [b]."""
    n = torch.minimum(nframes, int(stride) // channels.clamp(1, PCM_MAX_CHANNELS).long()).clamp_(min=0)
    return _tiled(n, tile_len) if tile_len > 0 else n


def raw_lengths(nframes, channels, fmt, byte_stride: int, rates=None, tile_secs: float = 0.0):
    """The lengths `pcm_ingest` will report, from the host's copies of a RawPcmBatch's arrays (no device sync) -> (n int64 [b],
    tile_len int64 [b] or None).  tile_secs > 0: every clip is tiled to int(tile_secs * its rate) samples."""
    width = torch.tensor(_ffi.PCM_WIDTH + (0,), dtype=torch.int64)[torch.where((fmt >= 0) & (fmt < 5), fmt, 5).long()]
    per = channels.clamp(1, PCM_MAX_CHANNELS).long() * width
    n = torch.where(per > 0, torch.minimum(nframes.long(), int(byte_stride) // per.clamp(min=1)), torch.zeros_like(per)).clamp_(min=0)
    if tile_secs <= 0 or rates is None:
        return n, None
    tile_len = torch.tensor([int(tile_secs * int(r)) for r in rates.tolist()], dtype=torch.int64)
    return _tiled(n, tile_len), tile_len


def clip_waves(clips, device, mode: str = "first", tile_secs: float = 0.0):
    """The one ingest door of the trainers: a PcmBatch or a RawPcmBatch on the host -> (wave fp32 [b, longest rounded up to 8],
    nsamples int64 [b] on the device, the same lengths on the host, the clips' rates on the host -- None for a PcmBatch, whose clips
    share one).  H2D without waiting, then `pcm_wave` or `pcm_ingest`; tile_secs > 0: every clip is tiled to int(tile_secs * its
    rate) samples.  The lengths come from the host's copies: nothing here synchronises with the device."""
    on_dev = clips.to(device, non_blocking=True)
    if isinstance(clips, RawPcmBatch):
        n, tile_len = raw_lengths(clips.nframes, clips.channels, clips.fmt, clips.raw.shape[1], clips.rates, tile_secs)
        wave, nsamples = pcm_ingest(on_dev.raw, on_dev.nframes, on_dev.channels, on_dev.fmt, mode=mode, tile_len=tile_len,
                                    wave_stride=max(8, -(-int(n.max()) // 8) * 8))
        return wave, nsamples, n, clips.rates
    tile_len = int(tile_secs * clips.sample_rate) if tile_secs > 0 else 0
    n = pcm_lengths(clips.nframes, clips.channels, clips.pcm.shape[1], tile_len)
    wave, nsamples = pcm_wave(on_dev.pcm, on_dev.nframes, on_dev.channels, mode=mode, tile_len=tile_len,
                              wave_stride=max(8, -(-int(n.max()) // 8) * 8))
    return wave, nsamples, n, None


class Resample:
    """Every clip of a batch to `target_rate`, on the device, in one launch (`vipant_resample`; `running.audio.resample_to`): the
    band-limited polyphase interpolation of torchaudio.functional.resample(waveform, rate, target_rate, lowpass_filter_width,
    rolloff) with its Hann-windowed sinc.  A rate pair is a class: its plan comes from the host
    (`vipant_resample_plan`; a pair whose table does not fit a workgroup's LDS, such as 44101 -> 16000, is refused there, when the
    object first sees the rate and before any launch), its table is built on the device when the pair first runs
    (`vipant_resample_table`) and kept.  A clip already at the target rate is copied bit for bit."""

    def __init__(self, target_rate: int, lowpass_filter_width: int = 6, rolloff: float = 0.99, device="cuda:0"):
        self.target_rate, self.width, self.rolloff = int(target_rate), int(lowpass_filter_width), float(rolloff)
        self.device = torch.device(device)
        if self.target_rate < 1:
            raise VipantError(f"resample: target rate {target_rate} Hz")
        self._plans, self._tables = {}, {}

    def plan(self, rate) -> "_ffi.ResampleClass":
        """The class descriptor of rate -> target_rate, without its table: o, n, T, w, P (the periods a workgroup owns: P n outputs
        from (P - 1) o + kspan inputs), kmin, kspan, lds_bytes.  Host only; raises for a pair the kernels refuse."""
        rate = int(rate)
        if rate not in self._plans:
            c = _ffi.ResampleClass()
            call("vipant_resample_plan", rate, self.target_rate, self.width, self.rolloff, _ffi.C.byref(c))
            self._plans[rate] = c
        return self._plans[rate]

    def _class(self, rate):
        rate, c = int(rate), self.plan(rate)
        if c.T and rate not in self._tables:
            nbytes = query("vipant_resample_table_bytes", rate, self.target_rate, self.width, self.rolloff)
            table = torch.empty(nbytes // 4, dtype=F32, device=self.device)
            call("vipant_resample_table", rate, self.target_rate, self.width, self.rolloff, table.data_ptr(), nbytes, ops._stream())
            self._tables[rate] = table
            c.table = table.data_ptr()
        return c

    def lengths(self, n, rates):
        """The lengths `__call__` will report, ceil(n_class * len / o_class), from the host's copies in Python integers (no device
        sync) -> int64 [b].  rates: one per row, or one for the batch."""
        n = torch.as_tensor(n).reshape(-1).tolist()
        rates = self._rates(rates, len(n))
        return torch.tensor([-(-self.plan(r).n * max(int(k), 0) // self.plan(r).o) for k, r in zip(n, rates)], dtype=torch.int64)

    @staticmethod
    def _rates(rates, b):
        rates = torch.as_tensor(rates).reshape(-1).tolist()
        if len(rates) == 1:
            rates = rates * b
        if len(rates) != b:
            raise VipantError(f"resample: {len(rates)} rates for {b} rows")
        return [int(r) for r in rates]

    def __call__(self, wave: torch.Tensor, nsamples: torch.Tensor, rates, host_lengths=None):
        """wave fp32 [b, stride] on the device, nsamples int64 [b] on the device, rates: host integers, one per row or one for the
        batch -> (wave_out fp32 [b, out_stride], zero beyond a clip's length; nsamples_out int64 [b]).  host_lengths: the host's copy
        of nsamples (as `clip_waves` returns it): out_stride is then the longest new length rounded up to 8; without it, the longest
        a row of `stride` samples can become.  Nothing here synchronises with the device."""
        if not isinstance(wave, torch.Tensor) or not wave.is_cuda or wave.dtype != F32 or wave.dim() != 2:
            raise VipantError("resample: wave must be a 2-d float32 device tensor (there is no CPU path)")
        wave = wave.contiguous()
        b, stride = wave.shape
        rates = self._rates(rates, b)
        groups = RateFbank.group(rates)
        if len(groups) > _ffi.RESAMPLE_MAX_CLASSES:
            raise VipantError(f"resample: a batch with {len(groups)} sample rates; one launch takes {_ffi.RESAMPLE_MAX_CLASSES}")
        classes = (_ffi.ResampleClass * len(groups))(*[self._class(rate) for rate, _ in groups])     # every refusal before the launch
        cls = (_ffi.C.c_int32 * b)()
        for k, (_, members) in enumerate(groups):
            for i in members:
                cls[i] = k
        longest = self.lengths(host_lengths if host_lengths is not None else [stride] * b, rates)
        out_stride = max(8, -(-int(longest.max()) // 8) * 8)
        nsamples = nsamples.to(device=wave.device, dtype=torch.int64).contiguous()
        if nsamples.shape != (b,):
            raise VipantError(f"resample: nsamples must have shape [{b}], got {tuple(nsamples.shape)}")
        out = torch.empty((b, out_stride), dtype=F32, device=wave.device)
        nout = torch.empty((b,), dtype=torch.int64, device=wave.device)
        call("vipant_resample", wave.data_ptr(), stride, nsamples.data_ptr(), cls, classes, len(groups), out.data_ptr(), out_stride,
             nout.data_ptr(), b, ops._stream())
        return out, nout


def fbank_config(acfg, train: bool = True) -> dict:
    """`acfg` = the reference's `running.audio` node (configs/running/audio/default.yaml) -> the constructor keywords that both
    filter banks read from it."""
    fm = tm = 0
    if train and getattr(acfg, "transform_fbank", False) and not getattr(acfg, "eval_norms", False):
        for name, params in getattr(acfg, "fbank_transforms", []):
            if name == "FrequencyMasking":
                fm = int(params[0])
            elif name == "TimeMasking":
                tm = int(params[0])
    norms = () if getattr(acfg, "eval_norms", False) else tuple(getattr(acfg, "norms", ()) or ())
    chain = ()
    if getattr(acfg, "transform_audio", False):
        chain = getattr(acfg, "audio_transforms", ()) or ()
        parse_audio_transforms(chain)           # a chain this front-end cannot run is an error wherever it is configured ...
        if not train or getattr(acfg, "eval_norms", False):
            chain = ()                          # ... and applies only to the training loader (image_audio.py:108-110)
    return dict(num_mel_bins=acfg.num_mel_bins, max_len=acfg.max_len, norms=norms, zero_mean_wf=getattr(acfg, "zero_mean_wf", True),
                frame_shift=getattr(acfg, "frame_shift", 10), freq_mask_param=fm, time_mask_param=tm, audio_transforms=chain,
                train=train)


class Fbank:
    """What `KaldiFbank` (one sample rate) and `RateFbank` (each clip's own) share: the settings, the host draws -- they do not depend
    on the rate --, the argument rules of `__call__` and the view plan.  A subclass says `crop_len_for(rate)`: the pipeline's crop
    length, int((max_len / 100 + 0.05) * rate) samples (transform.py:24-26)."""

    def __init__(self, num_mel_bins: int = 128, max_len: int = 1000, norms: Sequence[float] = (), zero_mean_wf: bool = True,
                 frame_shift: float = 10.0, frame_length: float = 25.0, preemphasis: float = 0.97, freq_mask_param: int = 0,
                 time_mask_param: int = 0, device="cuda:0", audio_transforms=(), train: bool = True):
        self.device = torch.device(device)
        self.num_mel_bins, self.max_len = int(num_mel_bins), int(max_len)
        self.norms = tuple(float(v) for v in norms) if len(norms) == 2 else ()
        self.zero_mean_wf, self.preemphasis = bool(zero_mean_wf), float(preemphasis)
        self.frame_shift, self.frame_length = float(frame_shift), float(frame_length)
        self.freq_mask_param, self.time_mask_param = int(freq_mask_param), int(time_mask_param)
        self.train = bool(train)                    # the pipeline's crop: drawn when training, centred otherwise
        self.chain = parse_audio_transforms(audio_transforms)

    def longer_than_crop(self, n, rates=None) -> bool:
        """Is a clip (n: the host's lengths; rates: one per clip, None where the bank has one) longer than the crop length of ITS rate?"""
        if rates is None:
            return int(n.max()) > self.crop_len_for(None)
        return any(int(k) > self.crop_len_for(int(r)) for k, r in zip(n.tolist(), rates.tolist()))

    def draw_masks(self, b: int, generator: Optional[torch.Generator] = None, *, freq_mask_param: Optional[int] = None,
                   time_mask_param: Optional[int] = None, sizes=None) -> Optional[torch.Tensor]:
        """[b, 4] int32 (f0, f1, t0, t1); mask_along_axis's draws: value = U*param, min = U*(size - value).
        freq_mask_param / time_mask_param override the object's own for this call (the siamese dataset's FbankTransform draws a
        prime set (32, 200) and a second set (48, 300) over one log-mel, transform.py:223-258); the generator is consumed alike.
        sizes: the time extent of every row (b integers) where it is not max_len -- a stored log-mel that the reference masks BEFORE it
        pads it has its own T_i rows (LogmelIngest.sizes) --; such a row's (t0, t1) is clamped into [0, size] (a clip shorter than
        the mask parameter, which mask_along_axis does not define).  None: max_len for every row and no clamp, the draws of before."""
        fparam = self.freq_mask_param if freq_mask_param is None else int(freq_mask_param)
        tparam = self.time_mask_param if time_mask_param is None else int(time_mask_param)
        if fparam <= 0 and tparam <= 0:
            return None
        if sizes is not None:
            sizes = [int(v) for v in (sizes.tolist() if isinstance(sizes, torch.Tensor) else sizes)]
            if len(sizes) != b:
                raise VipantError(f"fbank: draw_masks takes one size per row, got {len(sizes)} for {b} rows")
        rows = []
        for i in range(b):
            row = []
            for param, size in ((fparam, self.num_mel_bins), (tparam, self.max_len if sizes is None else sizes[i])):
                if param <= 0:
                    row += [0, 0]
                    continue
                value = torch.rand(1, generator=generator) * param
                min_value = torch.rand(1, generator=generator) * (size - value)
                start = int(min_value.long())
                row += [start, start + int(value.long())]
            if sizes is not None:
                row[2] = min(max(row[2], 0), sizes[i])
                row[3] = min(max(row[3], row[2]), sizes[i])
            rows.append(row)
        return torch.tensor(rows, dtype=torch.int32)

    @staticmethod
    def draw_mixup(b: int, rate: float, generator: Optional[torch.Generator] = None):
        """Mixup draws of one batch (cvap/data/audioset_cls.py:381-395, with the partner taken from the batch instead of the
        dataset): per clip one uniform draw against `rate`, a partner uniform in [0, b), lambda ~ Beta(10, 10) as the ratio of two
        Gamma(10) sums of exponentials.  -> (index int32 [b], -1 = not mixed; lambda fp32 [b], 1 where not mixed).  A clip that
        draws itself stays unmixed.  Every clip consumes the same number of draws, mixed or not."""
        u = torch.rand(b, generator=generator, dtype=torch.float64)
        partner = torch.randint(0, max(b, 1), (b,), generator=generator)
        e = -torch.log1p(-torch.rand(b, 20, generator=generator, dtype=torch.float64))      # Exp(1) draws; Gamma(10) = sum of 10
        ga, gb = e[:, :10].sum(1), e[:, 10:].sum(1)
        lam = (ga / (ga + gb)).to(F32)
        mixed = (u < float(rate)) & (partner != torch.arange(b))
        index = torch.where(mixed, partner, torch.full_like(partner, -1)).to(torch.int32)
        return index, torch.where(mixed, lam, torch.ones_like(lam))

    def draw_views(self, b: int, generator: Optional[torch.Generator] = None):
        """The draws of one batch for the waveform chain and the pipeline's crop -> (draws float64 [b, 6], seed int).
        draws[i] = (flip 0 / 1, scale factor, pad u, crop u, snr in dB or -1 for "no noise", final crop u): flip iff u <= p
        (transform.py:86), factor = scale ** U(-1, 1) (:101), the window positions as u in [0, 1) (left = floor(u * range), :127 /
        :158), noise iff u <= p with snr = u * (max - min + 1) + min (:187-189).  `seed` keys the noise generator.  Every clip
        consumes the same number of draws whatever fires, and a transform that is not in the chain leaves its neutral value."""
        u = torch.rand(b, 7, generator=generator, dtype=torch.float64)
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator))
        draws = torch.zeros(b, 6, dtype=torch.float64)
        draws[:, 1], draws[:, 4] = 1.0, -1.0
        draws[:, 2], draws[:, 3], draws[:, 5] = u[:, 2], u[:, 3], u[:, 6]
        if "RandomFlip" in self.chain:
            draws[:, 0] = (u[:, 0] <= float(self.chain["RandomFlip"]["p"])).double()
        if "RandomScale" in self.chain:
            draws[:, 1] = float(self.chain["RandomScale"]["scale"]) ** (2.0 * u[:, 1] - 1.0)
        if "RandomNoise" in self.chain:
            cfg = self.chain["RandomNoise"]
            lo, hi = float(cfg["snr_min_db"]), float(cfg["snr_max_db"])
            draws[:, 4] = torch.where(u[:, 4] <= float(cfg["p"]), u[:, 5] * (hi - lo + 1.0) + lo, draws[:, 4])
        return draws, seed

    @staticmethod
    def no_views(b: int):
        """The view that changes nothing and draws nothing -> (draws, seed): the value `draw_views` leaves where no transform fires,
        with the pipeline's window at the head (it only matters to a clip longer than `crop_len`)."""
        draws = torch.zeros(b, 6, dtype=torch.float64)
        draws[:, 1], draws[:, 4] = 1.0, -1.0
        return draws, 0

    def _view_args(self, view, b: int, n: int, dev, final_len: Optional[int] = None):
        """view = (draws, seed) or True -> (ViewParams, draws on the device).  final_len: the pipeline's crop length (default: the
        bank's one)."""
        if final_len is None:
            final_len = self.crop_len_for(None)
        if view is True:                            # the crop rule only: centred, or drawn from torch's default generator
            draws = torch.zeros(b, 6, dtype=torch.float64)
            draws[:, 1], draws[:, 4] = 1.0, -1.0
            if self.train:
                draws[:, 5] = torch.rand(b, dtype=torch.float64)
            seed, chain = 0, {}
        else:
            draws, seed = view
            chain = self.chain
            draws = torch.as_tensor(draws, dtype=torch.float64)
            if draws.shape != (b, 6):
                raise VipantError(f"fbank: view draws must have shape [{b}, 6], got {tuple(draws.shape)}")
        stages = pad_len = crop_len = 0
        padding_value = None
        if "RandomFlip" in chain:
            stages |= _ffi.VIEW_FLIP
        if "RandomScale" in chain:
            stages |= _ffi.VIEW_SCALE
            if n * max(float(chain["RandomScale"]["scale"]), 1.0) >= 2 ** 24:          # fp32 sample indices stop being exact
                raise VipantError(f"fbank: RandomScale of {n}-sample clips by up to {chain['RandomScale']['scale']} reaches 2^24 samples")
        if "RandomPad" in chain:
            cfg = chain["RandomPad"]
            stages |= _ffi.VIEW_PAD
            pad_len, padding_value = int(cfg["output_len"]), cfg["padding_value"]
        if "RandomCrop" in chain:
            cfg = chain["RandomCrop"]
            stages |= _ffi.VIEW_CROP
            crop_len = int(cfg["output_len"])
        if "RandomNoise" in chain:
            stages |= _ffi.VIEW_NOISE
        params = _ffi.ViewParams(pad_len, crop_len, int(final_len), int(seed) & (2 ** 64 - 1),
                                 float(padding_value) if padding_value is not None else 0.0, int(padding_value is not None),
                                 int(self.train), int(self.zero_mean_wf), stages, 0)
        return params, draws.to(dev).contiguous()

    def _wave_args(self, wave, nsamples):
        if not wave.is_cuda or wave.dtype != F32 or wave.dim() != 2:
            raise VipantError("fbank: wave must be a 2-d float32 device tensor (there is no CPU path)")
        wave = wave.contiguous()
        b, n = wave.shape
        if nsamples is None:
            nsamples = torch.full((b,), n, dtype=torch.int64, device=wave.device)
        return wave, nsamples.to(device=wave.device, dtype=torch.int64).contiguous()

    @staticmethod
    def _viewing(masks2, mix, view, pair) -> bool:
        """The argument refusals of `__call__`, before anything touches the device -> is there a view?"""
        viewing = view is not None and view is not False
        if pair and mix is not None:
            raise VipantError("fbank: `pair` and `mix` exclude each other (the two views of the siamese dataset are never mixed)")
        if pair and not viewing:
            raise VipantError("fbank: `pair` needs a view ((draws, seed), or True for the crop rule only)")
        if masks2 is not None and not pair:
            raise VipantError("fbank: `masks2` belongs to the second view of `pair=True`")
        if viewing and mix is not None:
            raise VipantError("fbank: `view` and `mix` exclude each other (the reference's clf loader mixes, its cst loader transforms)")
        return viewing

    @staticmethod
    def _output_rows(nsrc: int, mix, outputs) -> int:
        """-> b: the rows of wave that produce a log-mel (the rows past `outputs` are mixup partners)."""
        if outputs is None:
            return nsrc
        if mix is None:
            raise VipantError("fbank: `outputs` belongs to `mix` (the rows past it are mixup partners)")
        if not 1 <= int(outputs) <= nsrc:
            raise VipantError(f"fbank: outputs={outputs} outside [1, {nsrc}] (the rows of wave)")
        return int(outputs)

    @staticmethod
    def _on_device(dev, b: int, masks, masks2, mix, check_masks: bool):
        """masks / masks2 / mix as the launches read them -> (masks, masks2, index, lambda), each None where it was not given."""
        index = lam = None
        if masks is not None:
            masks = masks.to(device=dev, dtype=torch.int32).contiguous()
            if check_masks and masks.shape != (b, 4):
                raise VipantError(f"fbank: masks must have shape [{b}, 4] (one row per output), got {tuple(masks.shape)}")
        if masks2 is not None:
            masks2 = masks2.to(device=dev, dtype=torch.int32).contiguous()
        if mix is not None:
            index = mix[0].to(device=dev, dtype=torch.int32).contiguous()
            lam = mix[1].to(device=dev, dtype=F32).contiguous()
            if index.shape != (b,) or lam.shape != (b,):
                raise VipantError(f"fbank: mix index / lambda must have shape [{b}], got {tuple(index.shape)} / {tuple(lam.shape)}")
        return masks, masks2, index, lam


class KaldiFbank(Fbank):
    """kaldi.fbank(htk_compat=True, use_energy=False, window_type='hanning', dither=0, frame_shift=10) + dataset glue."""

    def __init__(self, sample_rate: float = 16000.0, num_mel_bins: int = 128, max_len: int = 1000,
                 norms: Sequence[float] = (), zero_mean_wf: bool = True, frame_shift: float = 10.0, frame_length: float = 25.0,
                 preemphasis: float = 0.97, freq_mask_param: int = 0, time_mask_param: int = 0, device="cuda:0",
                 audio_transforms=(), train: bool = True):
        super().__init__(num_mel_bins, max_len, norms, zero_mean_wf, frame_shift, frame_length, preemphasis, freq_mask_param,
                         time_mask_param, device, audio_transforms, train)
        self.sample_rate = float(sample_rate)
        self.crop_len = int((self.max_len / 100 + 0.05) * self.sample_rate)       # transform.py:24-26
        (self.shift, self.size, self.padded, self.window, self.banks, self.bank_start, self.bank_len) = _tables(
            self.sample_rate, self.num_mel_bins, frame_shift, frame_length, self.device)

    @classmethod
    def from_config(cls, acfg, sample_rate: float = 16000.0, train: bool = True, device="cuda:0"):
        """`acfg` = the reference's `running.audio` node (`fbank_config`)."""
        return cls(sample_rate, device=device, **fbank_config(acfg, train))

    def crop_len_for(self, rate=None) -> int:
        return self.crop_len

    def num_frames(self, num_samples: int) -> int:
        return 0 if num_samples < self.size else 1 + (num_samples - self.size) // self.shift

    def view_wave(self, wave: torch.Tensor, nsamples: Optional[torch.Tensor], view):
        """The waveform `__call__(..., view=view)` computes its filter bank from (`vipant_wave_view`: the same plan, the same sample
        function, the same bits) -> (wave_out fp32 [b, crop_len], zero beyond a clip's length; nsamples_out int64 [b])."""
        wave, nsamples = self._wave_args(wave, nsamples)
        b, n = wave.shape
        dev = wave.device
        params, draws = self._view_args(view, b, n, dev)
        out = torch.empty((b, self.crop_len), dtype=F32, device=dev)
        nout = torch.empty((b,), dtype=torch.int64, device=dev)
        ws = ops.scratch("fbank", query("vipant_fbank_view_workspace_bytes", b), dev)
        call("vipant_wave_view", wave.data_ptr(), n, nsamples.data_ptr(), out.data_ptr(), self.crop_len, nout.data_ptr(), b, params,
             draws.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        return out, nout

    def __call__(self, wave: torch.Tensor, nsamples: Optional[torch.Tensor] = None, masks: Optional[torch.Tensor] = None,
                 mix=None, view=None, masks2: Optional[torch.Tensor] = None, pair: bool = False, outputs: Optional[int] = None):
        """wave fp32 [b, n] on the device (rows zero-padded to a common n), nsamples int64 [b] valid lengths
        (default: n), masks int32 [b, 4] or None  ->  [b, 1, max_len, num_mel_bins] fp32.
        mix = (index int32 [b], lambda fp32 [b]) (draw_mixup): clip i becomes lambda c_i + (1 - lambda) c_index[i] on the
        zero-mean waveforms, inside the launch (vipant_fbank_mix; zero_mean_wf is implied, as in the reference's clf loader).
        outputs = b' (with mix): only rows 0 .. b'-1 of wave produce a log-mel; the rows past them are mixup partners from outside the
        batch, which index may point at (values in [-1, rows of wave)); index / lambda / masks have b' rows and the result is
        [b', 1, max_len, num_mel_bins] (vipant_fbank_mix_src when wave has more rows than b').
        view = (draws, seed) (draw_views): the waveform chain of `audio_transforms`, the pipeline's crop with its standard-deviation
        rule and the zero-mean, inside the launch (vipant_fbank_view); view = True: the crop rule only (centred when not training).
        `view` and `mix` exclude each other, as the reference's `cst` and `clf` loaders do (audioset_cls.py:374-432).
        pair = True (with a view): two views of the same log-mel that differ in their masks alone, from one filter-bank launch
        (vipant_fbank_view_pair) -> (out under `masks`, out2 under `masks2`), each [b, 1, max_len, num_mel_bins] with the bits the
        single call gives for its masks and the same view; either mask set may be None."""
        viewing = self._viewing(masks2, mix, view, pair)
        wave, nsamples = self._wave_args(wave, nsamples)
        nsrc, n = wave.shape
        dev = wave.device
        b = self._output_rows(nsrc, mix, outputs)
        masks, masks2, index, lam = self._on_device(dev, b, masks, masks2, mix, check_masks=outputs is not None)
        out = torch.empty((b, 1, self.max_len, self.num_mel_bins), dtype=F32, device=dev)
        mean, std = self.norms if self.norms else (0.0, 0.0)
        if mix is not None:
            if nsrc > b:                                         # partner rows past the batch: they are read, never written
                if nsamples.shape != (nsrc,):
                    raise VipantError(f"fbank: nsamples must have shape [{nsrc}], got {tuple(nsamples.shape)}")
                ws = ops.scratch("fbank", query("vipant_fbank_mix_src_workspace_bytes", nsrc, b), dev)
                call("vipant_fbank_mix_src", wave.data_ptr(), n, nsamples.data_ptr(), out.data_ptr(), self.window.data_ptr(),
                     self.banks.data_ptr(), self.bank_start.data_ptr(), self.bank_len.data_ptr(),
                     masks.data_ptr() if masks is not None else None, index.data_ptr(), lam.data_ptr(), nsrc, b, self.max_len,
                     self.num_mel_bins, self.size, self.shift, self.padded, self.preemphasis, float(mean), float(std),
                     ws.data_ptr(), ws.numel(), ops._stream())
                return out
            ws = ops.scratch("fbank", query("vipant_fbank_mix_workspace_bytes", b), dev)
            call("vipant_fbank_mix", wave.data_ptr(), n, nsamples.data_ptr(), out.data_ptr(), self.window.data_ptr(),
                 self.banks.data_ptr(), self.bank_start.data_ptr(), self.bank_len.data_ptr(),
                 masks.data_ptr() if masks is not None else None, index.data_ptr(), lam.data_ptr(), b, self.max_len,
                 self.num_mel_bins, self.size, self.shift, self.padded, self.preemphasis, float(mean), float(std), ws.data_ptr(),
                 ws.numel(), ops._stream())
            return out
        if pair:
            out2 = torch.empty_like(out)
            params, draws = self._view_args(view, b, n, dev)
            ws = ops.scratch("fbank", query("vipant_fbank_view_workspace_bytes", b), dev)
            call("vipant_fbank_view_pair", wave.data_ptr(), n, nsamples.data_ptr(), out.data_ptr(), out2.data_ptr(),
                 self.window.data_ptr(), self.banks.data_ptr(), self.bank_start.data_ptr(), self.bank_len.data_ptr(),
                 masks.data_ptr() if masks is not None else None, masks2.data_ptr() if masks2 is not None else None, b,
                 self.max_len, self.num_mel_bins, self.size, self.shift, self.padded, self.preemphasis, float(mean), float(std),
                 params, draws.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
            return out, out2
        if viewing:
            params, draws = self._view_args(view, b, n, dev)
            ws = ops.scratch("fbank", query("vipant_fbank_view_workspace_bytes", b), dev)
            call("vipant_fbank_view", wave.data_ptr(), n, nsamples.data_ptr(), out.data_ptr(), self.window.data_ptr(),
                 self.banks.data_ptr(), self.bank_start.data_ptr(), self.bank_len.data_ptr(),
                 masks.data_ptr() if masks is not None else None, b, self.max_len, self.num_mel_bins, self.size, self.shift,
                 self.padded, self.preemphasis, float(mean), float(std), params, draws.data_ptr(), ws.data_ptr(), ws.numel(),
                 ops._stream())
            return out
        ws = ops.scratch("fbank", query("vipant_fbank_workspace_bytes", b), dev)
        call("vipant_fbank", wave.data_ptr(), n, nsamples.data_ptr(), out.data_ptr(), self.window.data_ptr(),
             self.banks.data_ptr(), self.bank_start.data_ptr(), self.bank_len.data_ptr(),
             masks.data_ptr() if masks is not None else None, b, self.max_len, self.num_mel_bins, self.size, self.shift,
             self.padded, self.preemphasis, int(self.zero_mean_wf), float(mean), float(std), ws.data_ptr(), ws.numel(),
             ops._stream())
        return out


class RateFbank(Fbank):
    """`KaldiFbank` for a batch whose clips have different sample rates (`running.audio.native_pcm`).  The reference calls
    kaldi.fbank(sample_frequency=sr) with each file's own rate (cvap/data/audio/transform.py:15-35): a clip gets 25 ms / 10 ms frames
    at its rate and mel filters from 20 Hz to its Nyquist, and nothing is resampled.  Here the output rows are grouped by rate on the
    host and each rate class is one `vipant_fbank_rows` call -- its own window, mel weights and padded size (256 at 8 kHz ... 8192 at
    192 kHz) -- over the list of its rows, all into one [b, 1, T, F] result.  The table set of a rate is built when the rate is first
    seen (`_tables`).  The pipeline's crop length depends on the rate: crop_len(rate) = int((max_len / 100 + 0.05) * rate).  A mixup
    partner may have any rate: it is added sample by sample.  The constructor is `Fbank`'s: `KaldiFbank`'s without the rate."""

    MIN_PADDED, MAX_PADDED = 256, 8192

    @classmethod
    def from_config(cls, acfg, train: bool = True, device="cuda:0"):
        """`acfg` = the `running.audio` node, read exactly as `KaldiFbank.from_config` reads it (`fbank_config`)."""
        return cls(device=device, **fbank_config(acfg, train))

    def crop_len(self, rate) -> int:
        return int((self.max_len / 100 + 0.05) * float(rate))                     # transform.py:24-26, at the clip's own rate

    crop_len_for = crop_len

    def geometry(self, rate):
        """-> (shift, size, padded) of a rate's frames; raises for a rate whose window does not fit a padded size the kernels have."""
        rate = float(rate)
        shift, size = int(rate * self.frame_shift * 0.001), int(rate * self.frame_length * 0.001)
        padded = 1 << max(size - 1, 0).bit_length()
        if size < 2 or shift < 1 or not self.MIN_PADDED <= padded <= self.MAX_PADDED:
            raise VipantError(f"fbank: a clip with sample rate {int(rate)} Hz needs a {size}-sample window (padded to {padded}); the "
                              f"filter bank runs at padded sizes {self.MIN_PADDED} .. {self.MAX_PADDED} (there is no resampling)")
        return shift, size, padded

    @staticmethod
    def group(rates):
        """Host side: the rates of the output rows -> [(rate, [rows])], classes in the order of their first row."""
        classes = {}
        for i, r in enumerate(torch.as_tensor(rates).tolist()):
            classes.setdefault(int(r), []).append(i)
        return list(classes.items())

    def tables(self, rate):
        rate = int(rate)
        classes = self.__dict__.setdefault("_classes", {})
        if rate not in classes:
            self.geometry(rate)
            classes[rate] = _tables(float(rate), self.num_mel_bins, self.frame_shift, self.frame_length, self.device)
        return classes[rate]

    def __call__(self, wave: torch.Tensor, nsamples: torch.Tensor, rates, masks: Optional[torch.Tensor] = None, mix=None, view=None,
                 masks2: Optional[torch.Tensor] = None, pair: bool = False, outputs: Optional[int] = None):
        """The arguments of `KaldiFbank.__call__` plus rates: the sample rate of every output row (host integers; rows past
        `outputs` are mixup partners and their rates do not matter).  -> [b, 1, max_len, num_mel_bins] (two of them with pair)."""
        viewing = self._viewing(masks2, mix, view, pair)
        wave, nsamples = self._wave_args(wave, nsamples)
        nsrc, n = wave.shape
        dev = wave.device
        b = self._output_rows(nsrc, mix, outputs)
        if nsamples.shape != (nsrc,):
            raise VipantError(f"fbank: nsamples must have shape [{nsrc}], got {tuple(nsamples.shape)}")
        rates = torch.as_tensor(rates).reshape(-1)
        if rates.numel() < b:
            raise VipantError(f"fbank: {rates.numel()} rates for {b} output rows")
        classes = self.group(rates[:b])
        for rate, _ in classes:
            self.tables(rate)                           # every refusal before the first launch
        ptr = lambda t: t.data_ptr() if t is not None else None
        masks, masks2, index, lam = self._on_device(dev, b, masks, masks2, mix, check_masks=True)
        draws = params = None
        if viewing:                                     # the draws once for the batch; the pipeline's crop length per class below
            params, draws = self._view_args(view, b, n, dev, final_len=2)
        out = torch.empty((b, 1, self.max_len, self.num_mel_bins), dtype=F32, device=dev)
        out2 = torch.empty_like(out) if pair else None
        mean, std = self.norms if self.norms else (0.0, 0.0)
        rows = torch.tensor([i for _, members in classes for i in members], dtype=torch.int32).to(dev, non_blocking=True)
        ws = ops.scratch("fbank", query("vipant_fbank_rows_workspace_bytes", nsrc), dev)
        first = 0
        for rate, members in classes:
            shift, size, padded, window, banks, bank_start, bank_len = self.tables(rate)
            vp = None
            if viewing:
                vp = _ffi.ViewParams.from_buffer_copy(params)
                vp.final_len = self.crop_len(rate)
            desc = _ffi.FbankCall(
                wave.data_ptr(), n, nsamples.data_ptr(), out.data_ptr(), ptr(out2), window.data_ptr(), banks.data_ptr(),
                bank_start.data_ptr(), bank_len.data_ptr(), ptr(masks), ptr(masks2), ptr(index), ptr(lam),
                _ffi.C.pointer(vp) if vp is not None else None, ptr(draws), rows.data_ptr() + 4 * first, ws.data_ptr(), ws.numel(),
                nsrc, b, len(members), self.max_len, self.num_mel_bins, size, shift, padded, int(self.zero_mean_wf),
                self.preemphasis, float(mean), float(std), 0)
            call("vipant_fbank_rows", _ffi.C.byref(desc), ops._stream())
            first += len(members)
        return (out, out2) if pair else out


LOGMEL_KINDS = ("image_audio", "audioset_clf", "audioset")


def logmel_ingest(raw: torch.Tensor, nframes: torch.Tensor, fmt: torch.Tensor, max_len: int, num_mel_bins: int,
                  masks: Optional[torch.Tensor] = None, row_maxabs: bool = False, norms: Sequence[float] = (), pad_normed: bool = False):
    """Stored log-mels as their archives ship them -> the towers' input, in one launch (`vipant_logmel_ingest`): raw uint8
    [b, byte_stride] on the device, clip i = nframes[i] rows of num_mel_bins little-endian elements of format fmt[i] (_ffi.LOGMEL_F16 /
    F32 / F64); nframes / fmt are moved to the device, and nobody waits for them.  Per element in fp32: the row's max-abs division
    (row_maxabs), (x - mean) / std (norms), +0 or the normed zero (pad_normed) in the rows past a clip's end, +0 under the masks
    int32 [b, 4] = (f0, f1, t0, t1).  -> fp32 [b, max_len, num_mel_bins]."""
    if not isinstance(raw, torch.Tensor) or not raw.is_cuda:
        raise VipantError("logmel_ingest: raw must be a device tensor (there is no CPU path)")
    if raw.dtype != torch.uint8 or raw.dim() != 2:
        raise VipantError(f"logmel_ingest: raw must be a 2-d uint8 tensor, got {raw.dtype} {tuple(raw.shape)}")
    raw = raw.contiguous()
    b, stride = raw.shape
    dev = raw.device
    nframes = torch.as_tensor(nframes).to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
    fmt = torch.as_tensor(fmt).to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    if nframes.shape != (b,) or fmt.shape != (b,):
        raise VipantError(f"logmel_ingest: nframes / fmt must have shape [{b}], got {tuple(nframes.shape)} / {tuple(fmt.shape)}")
    if masks is not None:
        masks = torch.as_tensor(masks).to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
        if masks.shape != (b, 4):
            raise VipantError(f"logmel_ingest: masks must have shape [{b}, 4], got {tuple(masks.shape)}")
    norms = tuple(float(v) for v in norms) if norms is not None and len(norms) == 2 else ()
    if norms and norms[1] == 0.0:
        raise VipantError("logmel_ingest: norms with a zero standard deviation")
    mean, std = norms if norms else (0.0, 0.0)
    out = torch.empty((b, int(max_len), int(num_mel_bins)), dtype=F32, device=dev)
    call("vipant_logmel_ingest", raw.data_ptr(), stride, nframes.data_ptr(), fmt.data_ptr(), masks.data_ptr() if masks is not None else None,
         out.data_ptr(), b, int(max_len), int(num_mel_bins), int(bool(row_maxabs)), mean, std, int(bool(pad_normed)), ops._stream())
    return out


class LogmelIngest:
    """The step between a LogmelBatch (vipant_amd/data/npz.py) and the audio tower: what the reference's npz dataset classes do to a
    stored log-mel per item in numpy, for the batch on the device.  `dataset_kind` selects the order:
      image_audio   ImageAudioDatasetNpz (image_audio.py:71-79): masks over the clip's own T_i rows, zero pad; it reads no norms
      audioset_clf  AudiosetDatasetNpz (audioset_clf.py:91-103): `audio.normalized` row max-abs, norms, masks over T_i, zero pad
      audioset      AudiosetNpz (audioset_cls.py:173-183): pad, norms -- the padding is normed --, masks over max_len
    `running.audio.eval_norms` switches the norms off, as in the reference (and the masks, which the trainer draws)."""

    def __init__(self, num_mel_bins: int = 128, max_len: int = 1000, norms: Sequence[float] = (), row_maxabs: bool = False,
                 pad_normed: bool = False, mask_full_len: bool = False, device="cuda:0"):
        self.device = torch.device(device)
        self.num_mel_bins, self.max_len = int(num_mel_bins), int(max_len)
        self.norms = tuple(float(v) for v in norms) if norms is not None and len(norms) == 2 else ()
        self.row_maxabs, self.pad_normed, self.mask_full_len = bool(row_maxabs), bool(pad_normed), bool(mask_full_len)

    @classmethod
    def from_config(cls, acfg, train: bool = True, dataset_kind: str = "image_audio", device="cuda:0"):
        """`acfg` = the `running.audio` node.  (`train` changes nothing here: the masks are the trainer's to draw.)"""
        if dataset_kind not in LOGMEL_KINDS:
            raise VipantError(f"LogmelIngest: dataset kind `{dataset_kind}' is not one of {', '.join(LOGMEL_KINDS)}")
        norms = ()
        if dataset_kind != "image_audio" and not getattr(acfg, "eval_norms", False):
            norms = tuple(getattr(acfg, "norms", ()) or ())
        return cls(acfg.num_mel_bins, acfg.max_len, norms,
                   row_maxabs=dataset_kind == "audioset_clf" and bool(getattr(acfg, "normalized", False)),
                   pad_normed=dataset_kind == "audioset", mask_full_len=dataset_kind == "audioset", device=device)

    def sizes(self, nframes):
        """The time extent `draw_masks(sizes=)` takes per row, from the host's copy of the lengths: max_len where the reference masks
        the padded array, min(nframes, max_len) where it masks the stored one."""
        n = torch.as_tensor(nframes).reshape(-1).tolist()
        return [self.max_len if self.mask_full_len else max(0, min(int(k), self.max_len)) for k in n]

    def __call__(self, batch, masks: Optional[torch.Tensor] = None):
        """batch: a LogmelBatch (on the host or on the device) -> fp32 [b, 1, max_len, num_mel_bins]."""
        on_dev = batch.to(self.device, non_blocking=True)
        return logmel_ingest(on_dev.raw, on_dev.nframes, on_dev.fmt, self.max_len, self.num_mel_bins, masks=masks,
                             row_maxabs=self.row_maxabs, norms=self.norms, pad_normed=self.pad_normed).unsqueeze(1)
