"""The AudioSet tagging trainer's host side, without a GPU: the `+running=audioset` group against the reference's settings
(tests/golden/audioset_running.json, taken from configs/running/audioset.yaml), overrides, the soft-label arithmetic and mixup
draws, the two new entry points' ctypes rows against the header, BCELossHead's `soft_targets` switch, the synthetic loader."""
import ctypes as C
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = ("+running=audioset worker=ASClassifier monitor=ASMonitor +model/audio=vit_val +model/image=vit_val "
        "+model/text=transformer_val +model/loss=bce +optimizer=standard +running/audio=default")
LOCAL = ("clip_model_root", "data_root")          # the reference author's machine paths (blanked in the fixture): local defaults here


def _compose(extra=""):
    from vipant_amd.config import compose
    return compose(f"{LINE} {extra}".split())


def test_the_group_mirrors_the_reference_settings_key_for_key():
    from vipant_amd.config_defaults import GROUPS
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "audioset_running.json")))
    ours = GROUPS["running"]["audioset"]
    assert set(ref) <= set(ours), set(ref) - set(ours)
    for k, v in ref.items():
        if k not in LOCAL:
            assert ours[k] == v, (k, ours[k], v)
    assert (ours["clf"], ours["mixup_rate"], ours["imagine"], ours["zero_shot"], ours["save_rate"]) == (True, 0.5, False, False, 3)
    assert {k: ours[k] for k in ("synthetic_classes", "synthetic_steps", "synthetic_wave", "sample_rate")} == {
        "synthetic_classes": 527, "synthetic_steps": 8, "synthetic_wave": True, "sample_rate": 16000}


def test_the_launch_line_composes_and_overrides_parse():
    cfg = _compose()
    assert (cfg.worker, cfg.monitor, cfg.model.loss.name) == ("ASClassifier", "ASMonitor", "BCELossHead")
    r = cfg.running
    assert (r.batch_size, r.mixup_rate, r.max_audio_len, r.num_mel_bins, r.embed_dim) == (64, 0.5, 1000, 128, 512)
    assert list(r.excl_modules.amodules) == [] and list(r.excl_modules.vmodules) == []
    o = _compose("running.mixup_rate=0 running.synthetic_wave=False running.zero_shot=True running.synthetic_classes=12 "
                 "running.excl_modules.amodules=[pre_encoder] +model.loss.soft_targets=True").running
    assert (o.mixup_rate, o.synthetic_wave, o.zero_shot, o.synthetic_classes) == (0, False, True, 12)
    assert list(o.excl_modules.amodules) == ["pre_encoder"]
    import cvap.monitor
    import vipant_amd.monitor as VMon
    assert cvap.monitor.ASMonitor is VMon.ASMonitor is getattr(VMon, cfg.monitor) and "ASMonitor" in VMon.__all__


def test_soft_labels_and_mixup_draws_are_deterministic():
    from vipant_amd.frontend import KaldiFbank
    from vipant_amd.monitor import ASMonitor
    a = KaldiFbank.draw_mixup(32, 0.5, torch.Generator().manual_seed(9))
    b = KaldiFbank.draw_mixup(32, 0.5, torch.Generator().manual_seed(9))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    index, lam = a
    assert index.dtype == torch.int32 and lam.dtype == torch.float32 and 4 < int((index >= 0).sum()) < 28
    assert bool((index[index >= 0] != torch.arange(32)[index >= 0]).all()) and bool((lam[index < 0] == 1).all())
    assert bool((KaldiFbank.draw_mixup(8, 0.0, torch.Generator().manual_seed(1))[0] == -1).all())
    assert KaldiFbank.draw_mixup(1, 1.0, torch.Generator().manual_seed(1))[0].tolist() == [-1]
    # Beta(10, 10): mean 1/2, variance 1/84
    lam = KaldiFbank.draw_mixup(4000, 1.0, torch.Generator().manual_seed(2))[1]
    assert abs(float(lam.mean()) - 0.5) < 0.01 and abs(float(lam.var()) - 1 / 84) < 0.002
    y = torch.tensor([[1, 0, 1], [0, 1, 1], [0, 0, 1]])
    got = ASMonitor.soft_labels(y, torch.tensor([1, -1, 0], dtype=torch.int32), torch.tensor([0.25, 1.0, 0.5]))
    assert torch.equal(got, torch.tensor([[0.25, 0.75, 1.0], [0.0, 1.0, 1.0], [0.5, 0.0, 1.0]]))
    assert torch.equal(got, ASMonitor.soft_labels(y, torch.tensor([1, -1, 0], dtype=torch.int32), torch.tensor([0.25, 1.0, 0.5])))


_CTYPE = {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "size_t": C.c_size_t}


def _header_prototype(name):
    text = open(os.path.join(ROOT, "include", "vipant_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ret, args = re.search(rf"(\w+)\s+{name}\s*\(([^)]*)\)\s*;", text).groups()
    types = []
    for a in args.split(","):
        a = a.strip()
        types.append(C.c_void_p if "*" in a else _CTYPE[a.split()[-2]])
    return _CTYPE[ret], types


@pytest.mark.parametrize("name", ["vipant_fbank_mix", "vipant_fbank_mix_workspace_bytes", "vipant_bce_logits_soft"])
def test_ffi_rows_equal_the_header(name):
    from vipant_amd import _ffi
    assert _ffi.PROTOTYPES[name] == _header_prototype(name)
    # the same parser reproduces the rows of the entry points these were modelled on
    for known in ("vipant_fbank", "vipant_bce_logits"):
        assert _ffi.PROTOTYPES[known] == _header_prototype(known)
    assert _ffi.PROTOTYPES["vipant_bce_logits_soft"] == _ffi.PROTOTYPES["vipant_bce_logits"]


def test_host_checks_of_the_new_entry_points_run_without_a_gpu():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    assert _ffi.query("vipant_fbank_mix_workspace_bytes", 64) == 512 and _ffi.query("vipant_fbank_mix_workspace_bytes", 1) == 256
    ok = [16, 16000, 16, 16, 16, 16, 16, 16, None, 16, 16, 4, 128, 64, 400, 160, 512, 0.97, 0.0, 0.0, 16, 1 << 20, None]

    def refused(match, **change):
        args = list(ok)
        for i, v in change.items():
            args[int(i[1:])] = v
        with pytest.raises(_ffi.VipantError, match=match):
            _ffi.call("vipant_fbank_mix", *args)
    refused("null argument", a10=None)              # mix_lambda
    refused("null argument", a9=None)               # mix_index
    refused("bad batch", a11=0)
    refused("padded window", a16=500)
    refused("workspace", a21=16)
    with pytest.raises(_ffi.VipantError, match="dscale needs logit_scale"):
        _ffi.call("vipant_bce_logits_soft", 16, 64, 16, 64, None, 16, None, 64, 16, None, 0, 0, 8, 1.0, 8, 50, 16, 1 << 20, None)
    with pytest.raises(_ffi.VipantError, match="bce_logits_soft: bad shape"):
        _ffi.call("vipant_bce_logits_soft", 16, 64, 16, 64, None, 16, None, 64, None, None, 0, 0, 8, 1.0, 8, 65, 16, 1 << 20, None)


def test_bce_head_reads_soft_targets_from_its_config():
    import vipant_amd.module as M
    from vipant_amd.config import to_config
    base = {"name": "BCELossHead", "embed_dim": 512, "width": 768, "layers": [], "scaling": True, "bias": False}
    plain = M.build_loss_head(to_config(base), output_dim=12)
    soft = M.build_loss_head(to_config(dict(base, soft_targets=True)), output_dim=12)
    assert plain.soft_targets is False and soft.soft_targets is True
    assert M.build_loss_head(_compose().model.loss, output_dim=12).soft_targets is False
    assert list(plain.state_dict()) == list(soft.state_dict())                   # a switch, not a parameter or buffer
    y = torch.tensor([[0.0, 0.3, 1.0, 2.0]])
    cpu = torch.device("cpu")
    assert plain._target(y, cpu).dtype == torch.uint8 and plain._target(y, cpu).tolist() == [[0, 1, 1, 1]]
    assert soft._target(y, cpu).dtype == torch.float32 and torch.equal(soft._target(y, cpu), y)
    hot = torch.tensor([[0, 0, 1, 2]])
    for t in (hot, hot.bool(), hot.to(torch.uint8), hot.int()):                  # integer / bool targets stay binary either way
        assert soft._target(t, cpu).dtype == torch.uint8 and soft._target(t, cpu).bool().tolist() == [[False, False, True, True]]
    from vipant_amd import ops
    assert ops.ClassifierMeta("bce_soft", 12).kind == "bce_soft"
    with pytest.raises(AssertionError):
        ops.ClassifierMeta("soft", 12)


def test_synthetic_tagging_loader_contract():
    from vipant_amd.monitor import SyntheticTagging
    small = "running.batch_size=6 running.synthetic_classes=12 running.synthetic_steps=3 running.synthetic_seconds=0.5 " \
            "running.audio.max_len=64 running.audio.num_mel_bins=32"
    loader = SyntheticTagging(_compose(small), 3, True)
    assert len(loader) == 3 and len(loader.lid2int) == 12
    images, wave, nsamples, labels, names = next(iter(loader))
    assert images.shape == (6, 1, 1, 1) and wave.shape == (6, 8000) and wave.dtype == torch.float32
    assert nsamples.tolist() == [8000] * 6 and labels.shape == (6, 12) and labels.dtype == torch.int64 and len(names) == 6
    assert bool(((labels.sum(1) >= 1) & (labels.sum(1) <= 3)).all()) and set(labels.unique().tolist()) == {0, 1}
    assert torch.equal(wave, next(iter(loader))[1])                              # seeded per step
    batches = list(loader)
    assert len(batches) == 3 and not torch.equal(batches[0][1], batches[1][1])
    held = SyntheticTagging(_compose(small), 3, False)
    assert not torch.equal(next(iter(held))[1], wave) and next(iter(held))[4][0].startswith("synthetic-eval-")
    spec = SyntheticTagging(_compose(small + " running.synthetic_wave=False"), 3, True)
    images, audios, text, labels, names = next(iter(spec))
    assert audios.shape == (6, 64, 32) and text.shape == (6, 1) and labels.shape == (6, 12)
