"""GPU log-mel front-end: the step in front of the hot path.

The reference computes one Kaldi filter bank per clip on CPU dataloader workers
(cvap/data/audio/transform.py:12-35, parameters cvap/data/image_audio.py:119-126), pads / normalises it and applies
SpecAugment masks (image_audio.py:183-207, configs/running/audio/default.yaml).  `KaldiFbank` does the same for a whole
batch of device-resident waveforms in two launches (`vipant_fbank`; three with waveform mixup, `vipant_fbank_mix`) and returns the [b, 1, T, F] tensor
`ViTPreEncoder` takes.  With `outputs=b` the mixup partners may be rows of `wave` past the b clips of the batch (`vipant_fbank_mix_src`):
the file loader draws a partner from the whole dataset and ships its clip behind the batch; such a row is read, never written.  File decoding stays with the loader (vipant_amd/data); `pcm_wave` turns the 16-bit PCM it decodes into
those waveforms in one launch (`vipant_pcm_wave`: int16 -> fp32, the channel rule, `tile_audio`).  There is no resampling.

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


class KaldiFbank:
    """kaldi.fbank(htk_compat=True, use_energy=False, window_type='hanning', dither=0, frame_shift=10) + dataset glue."""

    def __init__(self, sample_rate: float = 16000.0, num_mel_bins: int = 128, max_len: int = 1000,
                 norms: Sequence[float] = (), zero_mean_wf: bool = True, frame_shift: float = 10.0, frame_length: float = 25.0,
                 preemphasis: float = 0.97, freq_mask_param: int = 0, time_mask_param: int = 0, device="cuda:0",
                 audio_transforms=(), train: bool = True):
        self.device = torch.device(device)
        self.sample_rate, self.num_mel_bins, self.max_len = float(sample_rate), int(num_mel_bins), int(max_len)
        self.norms = tuple(float(v) for v in norms) if len(norms) == 2 else ()
        self.zero_mean_wf, self.preemphasis = bool(zero_mean_wf), float(preemphasis)
        self.freq_mask_param, self.time_mask_param = int(freq_mask_param), int(time_mask_param)
        self.train = bool(train)                    # the pipeline's crop: drawn when training, centred otherwise
        self.chain = parse_audio_transforms(audio_transforms)
        self.crop_len = int((self.max_len / 100 + 0.05) * self.sample_rate)       # transform.py:24-26
        (self.shift, self.size, self.padded, self.window, self.banks, self.bank_start, self.bank_len) = _tables(
            self.sample_rate, self.num_mel_bins, frame_shift, frame_length, self.device)

    @classmethod
    def from_config(cls, acfg, sample_rate: float = 16000.0, train: bool = True, device="cuda:0"):
        """`acfg` = the reference's `running.audio` node (configs/running/audio/default.yaml)."""
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
        return cls(sample_rate, acfg.num_mel_bins, acfg.max_len, norms, getattr(acfg, "zero_mean_wf", True),
                   getattr(acfg, "frame_shift", 10), freq_mask_param=fm, time_mask_param=tm, device=device,
                   audio_transforms=chain, train=train)

    def num_frames(self, num_samples: int) -> int:
        return 0 if num_samples < self.size else 1 + (num_samples - self.size) // self.shift

    def draw_masks(self, b: int, generator: Optional[torch.Generator] = None, *, freq_mask_param: Optional[int] = None,
                   time_mask_param: Optional[int] = None) -> Optional[torch.Tensor]:
        """[b, 4] int32 (f0, f1, t0, t1); mask_along_axis's draws: value = U*param, min = U*(size - value).
        freq_mask_param / time_mask_param override the object's own for this call (the siamese dataset's FbankTransform draws a
        prime set (32, 200) and a second set (48, 300) over one log-mel, transform.py:223-258); the generator is consumed alike."""
        fparam = self.freq_mask_param if freq_mask_param is None else int(freq_mask_param)
        tparam = self.time_mask_param if time_mask_param is None else int(time_mask_param)
        if fparam <= 0 and tparam <= 0:
            return None
        rows = []
        for _ in range(b):
            row = []
            for param, size in ((fparam, self.num_mel_bins), (tparam, self.max_len)):
                if param <= 0:
                    row += [0, 0]
                    continue
                value = torch.rand(1, generator=generator) * param
                min_value = torch.rand(1, generator=generator) * (size - value)
                start = int(min_value.long())
                row += [start, start + int(value.long())]
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

    def _view_args(self, view, b: int, n: int, dev):
        """view = (draws, seed) or True -> (ViewParams, draws on the device)."""
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
        params = _ffi.ViewParams(pad_len, crop_len, self.crop_len, int(seed) & (2 ** 64 - 1),
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
        if pair and mix is not None:
            raise VipantError("fbank: `pair` and `mix` exclude each other (the two views of the siamese dataset are never mixed)")
        if pair and (view is None or view is False):
            raise VipantError("fbank: `pair` needs a view ((draws, seed), or True for the crop rule only)")
        if masks2 is not None and not pair:
            raise VipantError("fbank: `masks2` belongs to the second view of `pair=True`")
        if view is not None and view is not False and mix is not None:
            raise VipantError("fbank: `view` and `mix` exclude each other (the reference's clf loader mixes, its cst loader transforms)")
        wave, nsamples = self._wave_args(wave, nsamples)
        b, n = wave.shape
        dev = wave.device
        nsrc = b
        if outputs is not None:
            if mix is None:
                raise VipantError("fbank: `outputs` belongs to `mix` (the rows past it are mixup partners)")
            if not 1 <= int(outputs) <= nsrc:
                raise VipantError(f"fbank: outputs={outputs} outside [1, {nsrc}] (the rows of wave)")
            b = int(outputs)
        if masks is not None:
            masks = masks.to(device=dev, dtype=torch.int32).contiguous()
            if outputs is not None and masks.shape != (b, 4):
                raise VipantError(f"fbank: masks must have shape [{b}, 4] (one row per output), got {tuple(masks.shape)}")
        out = torch.empty((b, 1, self.max_len, self.num_mel_bins), dtype=F32, device=dev)
        mean, std = self.norms if self.norms else (0.0, 0.0)
        if mix is not None:
            index = mix[0].to(device=dev, dtype=torch.int32).contiguous()
            lam = mix[1].to(device=dev, dtype=F32).contiguous()
            if index.shape != (b,) or lam.shape != (b,):
                raise VipantError(f"fbank: mix index / lambda must have shape [{b}], got {tuple(index.shape)} / {tuple(lam.shape)}")
            if nsrc > b:                                            # partner rows past the batch: they are read, never written
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
            if masks2 is not None:
                masks2 = masks2.to(device=dev, dtype=torch.int32).contiguous()
            out2 = torch.empty_like(out)
            params, draws = self._view_args(view, b, n, dev)
            ws = ops.scratch("fbank", query("vipant_fbank_view_workspace_bytes", b), dev)
            call("vipant_fbank_view_pair", wave.data_ptr(), n, nsamples.data_ptr(), out.data_ptr(), out2.data_ptr(),
                 self.window.data_ptr(), self.banks.data_ptr(), self.bank_start.data_ptr(), self.bank_len.data_ptr(),
                 masks.data_ptr() if masks is not None else None, masks2.data_ptr() if masks2 is not None else None, b,
                 self.max_len, self.num_mel_bins, self.size, self.shift, self.padded, self.preemphasis, float(mean), float(std),
                 params, draws.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
            return out, out2
        if view is not None and view is not False:
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
