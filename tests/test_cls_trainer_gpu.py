"""ESCMonitor on the MI355X: two synthetic folds x two epochs of a 2-block tower train, the loss falls and the summary prints;
`eval=True running.zero_shot=True` prints a precision; a linear probe leaves the tower bit-identical."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

OV = ("+running=esc50 worker=ESClassifier monitor=ESCMonitor +model/audio=vit_val +model/image=vit_val "
      "+model/text=transformer_val +model/loss=ce_cls +optimizer=standard +running/audio=default num_gpus=1 "
      "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=2 model.text.encoder.layers=2 "
      "running.audio.max_len=256 running.audio.num_mel_bins=64 running.batch_size=16 running.epochs=2 "
      "running.synthetic_steps=2 running.synthetic_classes=8 running.peep_rate=1 optimizer.warmup_epoch=1 "
      "running.clip_model_root=/nonexistent")


def _monitor(extra):
    from vipant_amd.config import compose
    from vipant_amd.monitor import ESCMonitor
    cfg = compose((OV + " " + extra).split())
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    lines = []
    return ESCMonitor(cfg, lambda m: lines.append(str(m)), torch.device("cuda:0")), lines


@pytest.mark.timeout(600)
def test_two_folds_train_and_summarise():
    mon, lines = _monitor("eval=False")
    mon.learn()
    torch.cuda.synchronize()
    text = "\n".join(lines)
    assert text.count("Training started") == 2 and "Total 2 epochs for each of 2 folds." in text
    assert re.search(r"Best mean and std: \d+\.\d\d \\pm \d+\.\d\d in the \dth epoch\.", text), text
    assert re.search(r"Max mean and std: \d+\.\d\d \\pm \d+\.\d\d in the \[\d \d\]th epoch\.", text), text
    assert len(mon.report_by_fold) == 2 and all(len(r) == 2 for r in mon.report_by_fold)
    assert len(re.findall(r"A->T: p1 = \d+\.\d\d @ 32", text)) == 4
    # running mean of the loss, fold 0: after the first step and after the last (4 steps)
    means = [float(m) for m in re.findall(r"loss (\d+\.\d+) ", text)]
    print("[esc trainer] running loss per step:", means, "precision per fold and epoch:", mon.report_by_fold)
    assert len(means) == 8 and means[3] < means[0] and means[7] < means[4], means


@pytest.mark.timeout(600)
def test_zero_shot_evaluation_prints_a_precision():
    mon, lines = _monitor("eval=True running.zero_shot=True")
    assert not mon.model.training and mon.model.text_head is not None
    mon.learn()
    text = "\n".join(lines)
    assert re.search(r"A->T: p1 = \d+\.\d\d @ 64", text), text
    assert re.search(r"\d+\.\d\d for zero-shot classification\.", text), text


@pytest.mark.timeout(600)
def test_linear_probe_leaves_the_tower_bit_identical():
    mon, lines = _monitor("eval=False model.audio.freeze=True")
    assert "Freeze audio encoder." in lines
    tower = {k: v.detach().clone() for k, v in mon.model.audio_head.state_dict().items()}
    head = {k: v.detach().clone() for k, v in mon.model.loss_head.named_parameters()}
    _, loader = mon.loader_list[0][0]()
    from vipant_amd.module import adjust_learning_rate
    for step, batch in enumerate(loader):
        audios, labels, _ = mon.make_batch(batch)
        adjust_learning_rate(mon.cfg.optimizer, mon.optimizer, loader, step + 1)
        mon.step(audios, labels)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in mon.model.audio_head.parameters())
    assert all(p.grad is not None for p in mon.model.loss_head.parameters())
    for k, v in mon.model.audio_head.state_dict().items():
        assert torch.equal(v, tower[k]), k
    assert any(not torch.equal(p.detach(), head[k]) for k, p in mon.model.loss_head.named_parameters())
