"""Classification heads, workers and the ESC-50 trainer without a GPU: config groups through the launch-line parser, the
reference's module / state-dict layout (cvap/module/decoder/loss_head.py:330-419, loss_more.py:29-143), construction-time
refusals, the numpy restatement of the scikit-learn metrics, ESCMonitor.summary_report, the registries and the cvap.* aliases."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

LINE = ("+running=esc50 worker=ESClassifier monitor=ESCMonitor +model/audio=vit_val +model/image=vit_val "
        "+model/text=transformer_val +model/loss=ce_cls +optimizer=standard +running/audio=default")


def _compose(line=LINE, extra=""):
    from vipant_amd.config import compose
    return compose(f"{line} {extra}".split())


def test_the_launch_line_composes():
    cfg = _compose()
    assert cfg.worker == "ESClassifier" and cfg.monitor == "ESCMonitor"
    assert dict(cfg.model.loss) == {"name": "ClassificationHead", "embed_dim": 512, "layers": [], "scaling": True}
    r = cfg.running
    assert (r.batch_size, r.epochs, r.zero_shot, r.prompt, r.peep_rate) == (50, 32, False, "the sound of ", 16)
    assert list(r.excl_modules.amodules) == [] and r.synthetic_folds == 2 and cfg.optimizer.epochs == 32
    u = _compose(LINE.replace("esc50", "us8k")).running
    assert (u.data_name, u.peep_rate, u.batch_size, u.synthetic_classes) == ("UrbanSound8K", 50, 50, 10)
    b = _compose(LINE.replace("ce_cls", "bce")).model.loss
    assert dict(b) == {"name": "BCELossHead", "embed_dim": 512, "width": 768, "layers": [], "scaling": True, "bias": False}


def test_heads_build_with_the_reference_key_lists_and_load_strictly():
    import vipant_amd.module as M
    fx = np.load(os.path.join(GOLD, "cls_keys.npz"))
    ce = M.build_loss_head(_compose().model.loss, output_dim=50)
    assert isinstance(ce, M.ClassificationHead) and list(ce.state_dict()) == list(fx["keys_ce_cls"])
    assert list(ce.state_dict()) == ["logit_scale", "linear.0.weight", "linear.0.bias", "linear.1.weight", "linear.1.bias"]
    assert ce.normalized is False and ce.reduce is False and tuple(ce.linear[1].weight.shape) == (50, 512)
    assert abs(float(ce.logit_scale) - np.log(1 / 0.07)) < 1e-6
    b0 = M.build_loss_head(_compose(LINE.replace("ce_cls", "bce")).model.loss, output_dim=527)
    assert isinstance(b0, M.BCELossHead) and list(b0.state_dict()) == list(fx["keys_bce"]) and b0.linear[1].bias is None
    b1 = M.build_loss_head(_compose(LINE.replace("ce_cls", "bce"), "model.loss.layers=[256] model.loss.bias=True "
                                    "model.loss.scaling=False").model.loss, output_dim=527)
    assert list(b1.state_dict()) == list(fx["keys_bce_hidden"]) and "logit_scale" not in b1.state_dict()
    assert not isinstance(b1.logit_scale, torch.nn.Parameter) and float(b1.logit_scale) == 0.0
    assert [type(m).__name__ for m in b1.linear] == ["LayerNorm", "Linear", "LayerNorm", "Linear"]
    assert tuple(b1.linear[1].weight.shape) == (256, 512) and tuple(b1.linear[3].weight.shape) == (527, 256)
    for h in (ce, b0, b1):          # a reference-layout state dict loads strictly
        h.load_state_dict({k: torch.randn_like(v) for k, v in h.state_dict().items()}, strict=True)
    no_embed = _compose(LINE.replace("ce_cls", "bce"), "model.loss.embed_dim=null").model.loss       # embed_dim = cfg.embed_dim or cfg.width
    assert tuple(M.build_loss_head(no_embed, output_dim=5).linear[1].weight.shape) == (5, 768)


def test_copy_state_dict_semantics():
    """ClassificationHead copies every key it knows and ignores the rest; BCELossHead copies `logit_scale` alone and needs it."""
    import vipant_amd.module as M
    ce = M.build_loss_head(_compose().model.loss, output_dim=50)
    before = {k: v.clone() for k, v in ce.state_dict().items()}
    ce.copy_state_dict({"logit_scale": torch.tensor(1.5), "linear.1.bias": torch.full((50,), 2.0), "unknown.key": torch.zeros(3)})
    after = ce.state_dict()
    assert float(after["logit_scale"]) == 1.5 and bool((after["linear.1.bias"] == 2.0).all())
    assert torch.equal(after["linear.1.weight"], before["linear.1.weight"])
    b0 = M.build_loss_head(_compose(LINE.replace("ce_cls", "bce")).model.loss, output_dim=12)
    w = b0.linear[1].weight.detach().clone()
    b0.copy_state_dict({"logit_scale": torch.tensor(0.25), "linear.1.weight": torch.zeros_like(w)})
    assert float(b0.logit_scale) == 0.25 and torch.equal(b0.linear[1].weight, w)
    with pytest.raises(KeyError):
        b0.copy_state_dict({"linear.1.weight": w})


def test_bad_widths_and_missing_class_count_are_refused():
    import vipant_amd.module as M
    from vipant_amd._ffi import VipantError
    with pytest.raises(VipantError, match="embed_dim = 500 is not a positive multiple of 64"):
        M.build_loss_head(_compose(extra="model.image.embed_dim=500").model.loss, output_dim=50)
    with pytest.raises(VipantError, match=r"layers\[0\] = 100 is not a positive multiple of 64"):
        M.build_loss_head(_compose(LINE.replace("ce_cls", "bce"), "model.loss.layers=[100]").model.loss, output_dim=527)
    with pytest.raises(VipantError, match=r"layers\[0\] = 320 is not a multiple of 256"):
        M.build_loss_head(_compose(LINE.replace("ce_cls", "bce"), "model.loss.layers=[320]").model.loss, output_dim=527)
    with pytest.raises(VipantError, match="output_dim"):
        M.build_loss_head(_compose().model.loss)
    head = M.build_loss_head(_compose().model.loss, output_dim=50).train()
    with pytest.raises(VipantError, match="no CPU fallback"):
        head(torch.zeros(8, 512), torch.zeros(8, dtype=torch.int64))


def test_abi_queries_and_host_checks_run_without_a_gpu():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    assert _ffi.query("vipant_softmax_ce_workspace_bytes", 50) == 13 * 2 * 4
    assert _ffi.query("vipant_bce_logits_workspace_bytes", 4096) == 1024 * 2 * 4
    with pytest.raises(_ffi.VipantError, match="row range"):
        _ffi.call("vipant_softmax_ce", 16, 64, 16, 16, 16, None, 64, None, None, 4, 8, 1.0, 8, 50, 16, 1 << 20, None)
    with pytest.raises(_ffi.VipantError, match="workspace"):
        _ffi.call("vipant_softmax_ce", 16, 64, 16, 16, 16, None, 64, None, None, 0, 8, 1.0, 8, 50, None, 0, None)
    with pytest.raises(_ffi.VipantError, match="dscale needs logit_scale"):
        _ffi.call("vipant_bce_logits", 16, 64, 16, 64, None, 16, None, 64, 16, None, 0, 0, 8, 1.0, 8, 50, 16, 1 << 20, None)
    assert build.resource_usage().get("classify.hip"), "classify.hip is not part of the build"


def _random_problem(n, c, seed, ties):
    rng = np.random.default_rng(seed)
    y = rng.random((n, c)) < 0.15
    y[0], y[1] = True, False                     # every class has a positive and a negative
    s = rng.random((n, c)).astype(np.float32)
    return y, (np.round(s, 1) if ties else s)


@pytest.mark.parametrize("ties", [False, True])
def test_numpy_metrics_equal_scikit_learn(ties):
    sk = pytest.importorskip("sklearn.metrics")
    from vipant_amd.util import metrics as m
    y, s = _random_problem(300, 9, 5, ties)
    for avg in ("micro", "macro", "weighted"):
        assert abs(m.average_precision_score(y, s, avg) - sk.average_precision_score(y, s, average=avg)) <= 1e-12, avg
    for k in range(y.shape[1]):
        assert abs(m.average_precision(y[:, k], s[:, k]) - sk.average_precision_score(y[:, k], s[:, k])) <= 1e-12
        assert abs(m.roc_auc(y[:, k], s[:, k]) - sk.roc_auc_score(y[:, k], s[:, k])) <= 1e-12
        p, r, t = m.precision_recall_curve(y[:, k], s[:, k])
        p2, r2, t2 = sk.precision_recall_curve(y[:, k], s[:, k])
        assert p.shape == p2.shape and np.abs(p - p2).max() <= 1e-12 and np.abs(r - r2).max() <= 1e-12 and np.array_equal(t, t2)


def test_report_string_of_the_fixture_scores_is_reproduced_exactly():
    sys.path.insert(0, GOLD)
    import gen_cls
    from vipant_amd.util.metrics import multilabel_report
    fx = np.load(os.path.join(GOLD, "cls_reports.npz"))
    q = np.concatenate([np.load(os.path.join(GOLD, f"bce_scores{i}.npz"))["scores"] for i in (0, 1)]).astype(np.float32)
    _, Y = gen_cls.bce_inputs("bce_as", 1054, 527, part="eval")
    report = multilabel_report(Y.numpy(), q)
    assert report == str(fx["report_bce_as"]), (report, str(fx["report_bce_as"]))
    assert "Err(False)" in report and report.endswith("@ 1054")


def test_a_class_without_positives_or_negatives_sets_err_and_counts_zero():
    from vipant_amd.util import metrics as m
    y, s = _random_problem(40, 4, 1, False)
    y[:, 1] = False                               # no positive: AP 0, AUC counted 0
    y[:, 2] = True                                # no negative: AUC counted 0
    report = m.multilabel_report(y, s)
    assert "Err(True)" in report and report.endswith("@ 40")
    auc = [m.roc_auc(y[:, k], s[:, k]) for k in (0, 3)]
    assert f"mAUC = {np.mean(auc + [0.0, 0.0]) * 100.:2.2f}" in report
    assert m.average_precision(y[:, 1], s[:, 1]) == 0.0
    with pytest.raises(ValueError):
        m.roc_auc(y[:, 2], s[:, 2])


def test_summary_report_text():
    from vipant_amd.monitor import ESCMonitor
    lines = []
    mon = ESCMonitor.__new__(ESCMonitor)
    mon.echo = lines.append
    mon.summary_report([[10.0, 40.0, 30.0], [20.0, 30.0, 50.0]])
    assert lines[1] == "Total 3 epochs for each of 2 folds."
    assert lines[2] == "Best mean and std: 40.00 \\pm 10.00 in the 2th epoch."
    assert lines[3] == "Max mean and std: 45.00 \\pm 5.00 in the [1 2]th epoch."


def test_synthetic_folds_contract():
    from vipant_amd.monitor import SyntheticFolds
    cfg = _compose(extra="running.audio.max_len=64 running.audio.num_mel_bins=32 running.batch_size=10")
    data = SyntheticFolds(cfg, nfold=3, nclass=5, per_fold=20)
    assert len(data.loader_list) == 3 and len(data.lid2str) == 5 and len(data.lid2int) == 5
    _, train = data.loader_list[0][0]()
    _, held = data.loader_list[0][1]()
    assert len(train) == 4 and len(held) == 2
    audios, labels, names = next(iter(held))
    assert audios.shape == (10, 64, 32) and labels.dtype == torch.int64 and len(names) == 10
    assert labels.tolist() == [i % 5 for i in range(10)] and names[0] == "synthetic-fold0-0"
    again = next(iter(data.loader_list[0][1]()[1]))
    assert torch.equal(audios, again[0])
    seen = {n for b in train for n in b[2]}
    assert len(seen) == 40 and not any(n.startswith("synthetic-fold0-") for n in seen)
    first, second = [b[2] for b in train], [b[2] for b in train]
    assert first != second                       # reshuffled every epoch


def test_registries_resolve_through_the_reference_import_paths():
    import cvap.model
    import cvap.module
    import cvap.monitor
    import vipant_amd.model as VM
    import vipant_amd.monitor as VMon
    assert cvap.model.VAL_MODELS_REGISTRY.get("ESClassifier") is VM.ESClassifier is cvap.model.ESClassifier
    assert cvap.model.VAL_MODELS_REGISTRY.get("ASClassifier") is VM.ASClassifier is cvap.model.ASClassifier
    assert cvap.monitor.ESCMonitor is VMon.ESCMonitor
    reg = cvap.module.LOSS_HEADS_REGISTRY
    assert reg.get("ClassificationHead") is cvap.module.ClassificationHead and reg.get("BCELossHead") is cvap.module.BCELossHead
    for name in ("BCHingeLossHead", "ImagineAndClassifyLossHead", "LMLossHead"):
        assert name not in reg
    sys.path.insert(0, ROOT)
    import train  # noqa: F401
    assert getattr(VMon, _compose().monitor) is VMon.ESCMonitor


def test_models_build_on_a_cpu_host():
    """ESClassifier / ASClassifier construct (from scratch: no checkpoint, no CLIP file) and name their tunable parameters."""
    from vipant_amd.model import build_main_model
    small = ("eval=False model.image.encoder.layers=1 running.audio.max_len=64 running.audio.num_mel_bins=64 "
             "running.clip_model_root=/nonexistent")
    said = []
    cfg = _compose(extra=small + " running.excl_modules.amodules=[pre_encoder]")
    model = build_main_model(cfg, said.append)
    tunable = model.build(output_dim=50)
    assert any(k.startswith("loss_head.linear.1") for k in tunable) and "loss_head.logit_scale" in tunable
    assert any(k.startswith("audio_head.encoder.") for k in tunable) and not any(k.startswith("audio_head.pre_encoder.") for k in tunable)
    assert len(model.collect_audio_state_dict()) == 2
    probe = build_main_model(_compose(extra=small + " model.audio.freeze=True"), said.append)
    assert set(probe.build(output_dim=50)) == {f"loss_head.{k}" for k, _ in probe.loss_head.named_parameters()}
    assert "Freeze audio encoder." in said
    tag = build_main_model(_compose(LINE.replace("ce_cls", "bce").replace("ESClassifier", "ASClassifier"), small), said.append)
    tunable = tag.build(output_dim=527)
    assert "loss_head.linear.1.weight" in tunable and "loss_head.linear.1.bias" not in tunable
