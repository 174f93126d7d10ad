"""The host side of the waveform views (vipant_amd/frontend.py): which `running.audio.audio_transforms` chains are accepted, when
a chain applies, and the draws.  No GPU: the front-end's tables build on the CPU and nothing is launched."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED = "any subsequence of RandomFlip, RandomScale, RandomPad, RandomCrop, RandomNoise, in that order"


def acfg(transforms, **kw):
    base = dict(max_len=64, norms=[], eval_norms=False, num_mel_bins=64, zero_mean_wf=True, frame_shift=10, transform_audio=True,
                audio_transforms=transforms, transform_fbank=False, fbank_transforms=[])
    base.update(kw)
    return SimpleNamespace(**base)


def build(transforms, train=True, **kw):
    from vipant_amd.frontend import KaldiFbank
    return KaldiFbank.from_config(acfg(transforms, **kw), 16000.0, train=train, device="cpu")


@pytest.mark.parametrize("transforms,why", [
    ([["RandomScale", [1.5]], ["RandomFlip", [0.5]]], "`RandomFlip' is out of order"),
    ([["RandomNoise", [10, 120, 0.25]], ["RandomCrop", [44100]]], "`RandomCrop' is out of order"),
    ([["RandomFlip", [0.5]], ["RandomFlip", [0.5]]], "`RandomFlip' appears twice"),
    ([["SimpleRandomNoise", [10.0, 10, 0.25]]], "`SimpleRandomNoise' is not supported"),
    ([["RandomScale", [1.5, True]]], "keep_len=True"),
    ([["RandomScale", {"scale": 1.5, "keep_len": True}]], "keep_len=True"),
    ([["FrequencyMasking", [32]]], "`FrequencyMasking' is not supported"),
    ([["RandomFlip", [0.5, 1]]], "at most 1 parameters"),
    ([["RandomNoise", {"snr": 3}]], "no parameter `snr'"),
    ([["RandomPad", [88200, False]]], "RandomPad(train=False)"),
    ([["RandomCrop", {"output_len": 44100, "train": False}]], "RandomCrop(train=False)"),
])
def test_refused_chains_raise_and_name_the_accepted_chain(transforms, why):
    from vipant_amd._ffi import VipantError
    for train in (True, False):                                   # an error wherever it is configured, not a silent skip
        with pytest.raises(VipantError) as e:
            build(transforms, train=train)
        assert why in str(e.value) and ACCEPTED in str(e.value), str(e.value)


def test_dict_and_list_parameter_forms():
    full = [["RandomFlip", [0.3]], ["RandomScale", {"scale": 1.25}], ["RandomPad", [88200, True, 0.0]],
            ["RandomCrop", {"output_len": 44100}], ["RandomNoise", {"snr_max_db": 60.0, "p": 0.5}]]
    fb = build(full)
    assert list(fb.chain) == ["RandomFlip", "RandomScale", "RandomPad", "RandomCrop", "RandomNoise"]
    assert fb.chain["RandomFlip"] == {"p": 0.3} and fb.chain["RandomScale"] == {"scale": 1.25, "keep_len": False}
    assert fb.chain["RandomPad"] == {"output_len": 88200, "train": True, "padding_value": 0.0}
    assert fb.chain["RandomCrop"] == {"output_len": 44100, "train": True}
    assert fb.chain["RandomNoise"] == {"snr_min_db": 10.0, "snr_max_db": 60.0, "p": 0.5}
    assert fb.crop_len == int((64 / 100 + 0.05) * 16000) == 11040 and fb.train is True
    for sub in ([], [full[1]], [full[0], full[4]], [full[2], full[3]], [["RandomScale", []]]):
        assert list(build(sub).chain) == [t[0] for t in sub]
    # the project's own config nodes (a composed command line) take the same road
    sys.path.insert(0, ROOT)
    from vipant_amd.config import compose
    cfg = compose(("+running=audioset worker=ASClassifier monitor=ASMonitor +model/audio=vit_val +model/image=vit_val "
                   "+model/text=transformer_val +model/loss=bce +optimizer=standard +running/audio=default num_gpus=1 "
                   "running.audio.transform_audio=True running.audio.audio_transforms=[[RandomScale,[1.25]],[RandomNoise,[10,120,0.25]]]").split())
    from vipant_amd.frontend import KaldiFbank
    fb = KaldiFbank.from_config(cfg.running.audio, 16000.0, train=True, device="cpu")
    assert fb.chain == {"RandomScale": {"scale": 1.25, "keep_len": False}, "RandomNoise": {"snr_min_db": 10, "snr_max_db": 120, "p": 0.25}}
    assert fb.crop_len == 160800


def test_the_chain_applies_only_to_the_training_loader():
    chain = [["RandomScale", [1.5]], ["RandomNoise", [10, 120, 0.25]]]
    assert list(build(chain).chain) == ["RandomScale", "RandomNoise"]
    assert build(chain, train=False).chain == {} and build(chain, train=False).train is False
    assert build(chain, eval_norms=True).chain == {}
    assert build(chain, transform_audio=False).chain == {}
    assert build([["SimpleRandomNoise", []]], transform_audio=False).chain == {}      # not configured: not parsed


def test_draw_views():
    full = [["RandomFlip", [0.5]], ["RandomScale", [1.5]], ["RandomPad", [88200]], ["RandomCrop", [44100]], ["RandomNoise", [10.0, 120.0, 0.25]]]
    fb = build(full)
    n = 4000
    a, seed_a = fb.draw_views(n, torch.Generator().manual_seed(3))
    b, seed_b = fb.draw_views(n, torch.Generator().manual_seed(3))
    assert torch.equal(a, b) and seed_a == seed_b and isinstance(seed_a, int) and 0 <= seed_a < 2 ** 62
    assert a.shape == (n, 6) and a.dtype == torch.float64
    other, seed_o = fb.draw_views(n, torch.Generator().manual_seed(4))
    assert not torch.equal(a, other) and seed_o != seed_a
    flip, scale, pad_u, crop_u, snr, final_u = a.unbind(1)
    assert set(flip.tolist()) == {0.0, 1.0}
    assert abs(float(flip.mean()) - 0.5) < 5 * (0.25 / n) ** 0.5                                  # Bernoulli(0.5), 5 sigma
    noisy = snr >= 0
    assert abs(float(noisy.double().mean()) - 0.25) < 5 * (0.25 * 0.75 / n) ** 0.5                # Bernoulli(0.25), 5 sigma
    assert bool((snr[~noisy] == -1).all()) and bool(((snr[noisy] >= 10.0) & (snr[noisy] < 131.0)).all())
    assert float(snr[noisy].max()) > 120.0                                                        # u * (max - min + 1) + min, as the reference
    assert bool(((scale >= 1 / 1.5) & (scale <= 1.5)).all()) and float(scale.min()) < 0.7 and float(scale.max()) > 1.45
    assert abs(float(scale.log().mean())) < 5 * (torch.log(torch.tensor(1.5)).item() / 3 ** 0.5) / n ** 0.5   # log-uniform about 1
    for u in (pad_u, crop_u, final_u):
        assert bool(((u >= 0) & (u < 1)).all()) and abs(float(u.mean()) - 0.5) < 5 * (1 / 12 / n) ** 0.5
    # every clip consumes the same number of draws whatever fires: the generator ends in the same state for any chain, and the
    # draws of a stage do not move when another stage is taken out
    states = []
    for sub in (full, [full[0]], [full[4]], []):
        g = torch.Generator().manual_seed(3)
        d, s = build(sub).draw_views(n, g)
        states.append(g.get_state())
        assert s == seed_a and torch.equal(d[:, [2, 3, 5]], a[:, [2, 3, 5]])
        if sub and sub[0][0] == "RandomFlip":
            assert torch.equal(d[:, 0], flip)
        if sub and sub[-1][0] == "RandomNoise":
            assert torch.equal(d[:, 4], snr)
    assert all(torch.equal(s, states[0]) for s in states)
    none, _ = build([]).draw_views(8, torch.Generator().manual_seed(1))
    assert bool((none[:, 0] == 0).all()) and bool((none[:, 1] == 1).all()) and bool((none[:, 4] == -1).all())


def test_view_arguments():
    from vipant_amd import _ffi
    from vipant_amd._ffi import VipantError
    fb = build([["RandomFlip", [0.5]], ["RandomScale", [1.5]], ["RandomPad", {"output_len": 88200, "padding_value": 0.5}],
                ["RandomCrop", [44100, True]], ["RandomNoise", []]])
    draws, seed = fb.draw_views(2, torch.Generator().manual_seed(1))
    p, d = fb._view_args((draws, seed), 2, 16000, torch.device("cpu"))
    assert p.stages == 31 and (p.pad_len, p.crop_len, p.final_len) == (88200, 44100, 11040) and p.seed == seed
    assert p.has_padding_value == 1 and p.padding_value == 0.5 and p.train == 1 and p.zero_mean == 1 and torch.equal(d, draws)
    p, d = fb._view_args(True, 2, 16000, torch.device("cpu"))                   # the crop rule only
    assert p.stages == 0 and p.final_len == 11040 and d[:, :5].tolist() == [[0.0, 1.0, 0.0, 0.0, -1.0]] * 2
    p, d = build([], train=False)._view_args(True, 2, 16000, torch.device("cpu"))
    assert p.train == 0 and d[:, 5].tolist() == [0.0, 0.0]
    with pytest.raises(VipantError, match="2\\^24"):
        fb._view_args((torch.zeros(1, 6), 0), 1, 12000000, torch.device("cpu"))
    assert _ffi.VIEW_FLIP | _ffi.VIEW_SCALE | _ffi.VIEW_PAD | _ffi.VIEW_CROP | _ffi.VIEW_NOISE == 31
    assert _ffi.query("vipant_fbank_view_workspace_bytes", 512) == 512 * 64 and _ffi.query("vipant_fbank_view_workspace_bytes", 1) == 256
    with pytest.raises(VipantError, match="no CPU path"):
        fb(torch.zeros(2, 16000), view=True)


def test_registry_names_and_exclusions_are_unchanged():
    """tests/test_cls_cpu.py:195's: this feature adds no loss head and takes none away."""
    sys.path.insert(0, ROOT)
    import cvap.module
    reg = cvap.module.LOSS_HEADS_REGISTRY
    assert reg.get("ClassificationHead") is cvap.module.ClassificationHead and reg.get("BCELossHead") is cvap.module.BCELossHead
    for name in ("BCHingeLossHead", "ImagineAndClassifyLossHead", "LMLossHead"):
        assert name not in reg
