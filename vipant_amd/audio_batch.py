"""The trainers' audio batch path: a loader's clips on the host -> log-mels [b, 1, T, F] on the device (DESIGN.md sections 17-21, 28).
`AudioBatches` is built from `running.audio`, the device and a per-rank seed and knows no model: whether training is on is an argument
of every call.  One method per batch the reference's datasets make, each for a PcmBatch (one sample rate: `pcm_wave`, `KaldiFbank`)
and a RawPcmBatch (`running.audio.native_pcm`: `pcm_ingest`, `RateFbank`) alike, and each the one place that states the order of its
host draws -- a parity contract with the reference that the trainer tests replay from an identically seeded generator.
With `running.audio.resample_to` (a rate in Hz; 0 = off) every method brings its clips to that rate first (`frontend.Resample`, one
launch per batch, mixup partners included) and runs the `KaldiFbank` of that rate: crop length, masks and views live there."""
from __future__ import annotations

import torch

from . import frontend
from .frontend import KaldiFbank, LogmelIngest, RateFbank, Resample

# FbankTransform's own normalisation (cvap/data/audio/transform.py:228-229, :238-239, :247-248): the siamese dataset does not read
# `running.audio.norms`
FBANK_NORMS = (-4.93839311, 5.75751113)
PRIME_MASKS = (32, 200)         # transform_prime: FrequencyMasking(32), TimeMasking(200) -> view 1
SECOND_MASKS = (48, 300)        # transform: FrequencyMasking(48), TimeMasking(300) -> view 2


class AudioBatches:
    def __init__(self, acfg, device, seed: int):
        self.acfg, self.device, self.seed = acfg, device, int(seed)
        self._generator = None
        self._frontends = {}

    def fresh_generator(self):
        """A generator of the waveform-view, mixup and SpecAugment draws, at its seed."""
        return torch.Generator().manual_seed(self.seed)

    @property
    def generator(self):
        """The host generator of the draws: seeded per rank, created on first use, consumed in step order."""
        if self._generator is None:
            self._generator = self.fresh_generator()
        return self._generator

    @generator.setter
    def generator(self, generator):
        self._generator = generator

    def frontend(self, kind: str, train: bool, rate=None):
        """The front-ends, built on first use.  kind `config`: the filter bank `running.audio` describes; `siamese`: the siamese
        dataset's -- FbankTransform's constants, no chain, no masks of its own --; a LogmelIngest dataset kind: that ingest.
        rate: the sample rate of a PcmBatch (`KaldiFbank`), None for the clips' own (`RateFbank`)."""
        key = (kind, bool(train), None if rate is None else int(rate))
        if key not in self._frontends:
            self._frontends[key] = self._build(*key)
        return self._frontends[key]

    def _build(self, kind, train, rate):
        acfg = self.acfg
        if kind == "config":
            if rate is None:
                return RateFbank.from_config(acfg, train=train, device=self.device)
            return KaldiFbank.from_config(acfg, float(rate), train=train, device=self.device)
        if kind == "siamese":
            args = (acfg.num_mel_bins, acfg.max_len, FBANK_NORMS, acfg.get("zero_mean_wf", True), acfg.get("frame_shift", 10))
            cls, args = (RateFbank, args) if rate is None else (KaldiFbank, (float(rate),) + args)
            return cls(*args, device=self.device, train=train)
        return LogmelIngest.from_config(acfg, train=train, dataset_kind=kind, device=self.device)

    def _waves(self, kind, clips, train, mode="first", tile=False):
        """-> (the front-end of the clips' batch type, the positional arguments of its call, the host lengths, the rates or None).
        With `running.audio.resample_to`: the waveform as without it -- a clip is tiled at its own rate --, then all rows to that
        rate (skipped for a PcmBatch already there); the front-end is that rate's, the lengths are the new ones, the rates None."""
        to = int(self.acfg.get("resample_to", 0) or 0)
        fbank = self.frontend(kind, train, to if to else getattr(clips, "sample_rate", None))
        wave, nsamples, n, rates = frontend.clip_waves(clips, self.device, mode, fbank.max_len / 100 if tile else 0.0)
        if to:
            source = rates if rates is not None else clips.sample_rate
            if rates is not None or int(source) != to:
                resample = self.resampler(to)
                wave, nsamples = resample(wave, nsamples, source, host_lengths=n)
                n = resample.lengths(n, source)
            return fbank, (wave, nsamples), n, None
        return fbank, (wave, nsamples) if rates is None else (wave, nsamples, rates), n, rates

    def resampler(self, rate):
        """The `Resample` to `rate`, built on first use (it keeps the tables of the source rates it has seen)."""
        key = ("resample", int(rate))
        if key not in self._frontends:
            self._frontends[key] = Resample(int(rate), device=self.device)
        return self._frontends[key]

    def single_view(self, clips, train: bool, tile=None):
        """A PcmBatch / RawPcmBatch -> log-mels, in the reference's order (image_audio.py:183-207, transform.py:15-35): H2D, the
        waveform (channel rule, `tile_audio`), then inside the log-mel launch the `audio_transforms` chain and the crop rule, the
        filter bank, `norms`, and the SpecAugment masks.  `eval_norms` switches chain, masks and norms off.  `tile`: None follows
        `running.audio.tile_audio`; False never tiles (the x-fold datasets pass `tile_audio=False` whatever the key says, esc50.py:81).
        Draws: training -- `draw_views(b)` when there is a chain or a clip longer than its crop length, then `draw_masks(b)`;
        evaluation -- none (`view=True`, the centred window and its rule, for such a clip)."""
        tile = bool(self.acfg.get("tile_audio", False)) if tile is None else bool(tile)
        fbank, args, n, rates = self._waves("config", clips, train, str(self.acfg.get("channel", "first")), tile)
        b, view = n.shape[0], None
        crop = fbank.longer_than_crop(n, rates)
        if train and (fbank.chain or crop):
            view = fbank.draw_views(b, self.generator)
        elif crop:
            view = True
        masks = fbank.draw_masks(b, self.generator) if train else None
        return fbank(*args, masks=masks, view=view)

    def siamese_views(self, clips, train: bool, both: bool):
        """A PcmBatch / RawPcmBatch -> (view 1, view 2 or None) as the siamese dataset makes them (cvap/data/image_audio.py:256-285,
        transform.py:223-258): H2D, the waveform (channel 0, no tiling), then ONE log-mel launch that writes both views
        (`vipant_fbank_view_pair`).  No waveform chain whatever `running.audio.transform_audio` says (:238); the pipeline's crop of
        a clip longer than its crop length; `zero_mean_wf` from the config; FbankTransform's constants.  View 2 exists only when
        training with `both` (`model.loss.aa`); otherwise the single `vipant_fbank_view` launch.
        Draws: training -- `draw_views(b)` if a clip is longer than its crop length (else `no_views`, which draws nothing), then
        `draw_masks(b, *PRIME_MASKS)` for view 1, then with `both` `draw_masks(b, *SECOND_MASKS)` for view 2; evaluation -- none
        (`view=True`, view 1 unmasked)."""
        fbank, args, n, rates = self._waves("siamese", clips, train)
        b = n.shape[0]
        if not train:
            return fbank(*args, view=True), None
        view = fbank.draw_views(b, self.generator) if fbank.longer_than_crop(n, rates) else fbank.no_views(b)
        masks = fbank.draw_masks(b, self.generator, freq_mask_param=PRIME_MASKS[0], time_mask_param=PRIME_MASKS[1])
        if not both:
            return fbank(*args, masks=masks, view=view), None
        masks2 = fbank.draw_masks(b, self.generator, freq_mask_param=SECOND_MASKS[0], time_mask_param=SECOND_MASKS[1])
        return fbank(*args, masks=masks, view=view, masks2=masks2, pair=True)

    def tagging(self, clips, mix, train: bool):
        """The clips of a raw-file tagging batch -- b clips and, behind them, the partner clips the loader's workers drew
        (audioset_cls.py:374-400) -- and mix = (index, lambda) with b rows -> b log-mels: the waveform of all rows (channel 0, never
        tiled -- `wf[:1]`), then one launch that mixes and writes b rows.  The waveform is always zero-mean (:377), a longer clip is
        cut at `max_len` frames (:410); a partner of any rate is added sample by sample (under `resample_to` it has the batch's rate).
        Draws: training -- `draw_masks(b)` for the b outputs; evaluation -- none."""
        fbank, args, _, _ = self._waves("config", clips, train)
        b = int(mix[0].shape[0])
        masks = fbank.draw_masks(b, self.generator) if train else None
        return fbank(*args, masks=masks, mix=mix, outputs=b)

    def logmel(self, clips, train: bool, sample_rate):
        """A LogmelBatch (`running.npz_data`: stored log-mels as their archives hold them, on the host) -> [b, 1, T, F]: H2D of the
        bytes and one launch (`LogmelIngest`) that does what the reference's npz dataset does per item in numpy.
        Draws: training -- `draw_masks(b, sizes=)` of the configured filter bank at `sample_rate`, over each clip's own rows where
        the reference masks before it pads; evaluation -- none."""
        ingest, fbank = self.frontend(clips.kind, train), self.frontend("config", train, sample_rate)
        masks = fbank.draw_masks(clips.raw.shape[0], self.generator, sizes=ingest.sizes(clips.nframes)) if train else None
        return ingest(clips, masks)
