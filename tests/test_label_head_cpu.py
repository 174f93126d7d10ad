"""Host side of the label-aware InfoNCE head: config groups, name resolution, registries, the all-0-labels refusal, `ce_val` without the key."""
import pytest

import vipant_amd.module as M
from vipant_amd import monitor
from vipant_amd._ffi import VipantError
from vipant_amd.config import compose, to_config


def loss_cfg(name):
    return compose([f"+model/loss={name}"]).model.loss


def test_groups_compose_and_heads_resolve():
    import cvap.module
    ce, val, lab = loss_cfg("ce_label"), loss_cfg("ce_val"), loss_cfg("ce_val_label")
    assert dict(ce) == {"name": "LabelCELossHead", "layers": [], "scaling": True, "scale_max": None}
    assert dict(lab) == dict(val, label_positives=["al"]) and "label_positives" not in val
    head = cvap.module.build_loss_head(ce)
    assert type(head) is cvap.module.LabelCELossHead is M.MORE_LOSS_HEADS_REGISTRY.get("LabelCELossHead") and head.wants_groups
    assert issubclass(M.LabelCELossHead, M.CELossHead) and sorted(head.state_dict()) == ["logit_scale"]
    assert sorted(k for k, _ in M.LOSS_HEADS_REGISTRY) == ["BCELossHead", "BarlowCELossHead", "BarlowLossHead", "CELossHead", "ClassificationHead",
                                                          "DummyHead", "VACELossHead", "VALCELossHead"]
    plain, tri = M.build_loss_head(val), M.build_loss_head(lab)
    assert [type(h) for h in (plain.loss_head_va, plain.loss_head_lv, plain.loss_head_al)] == [M.CELossHead, type(None), M.CELossHead]
    assert [type(h) for h in (tri.loss_head_va, tri.loss_head_lv, tri.loss_head_al)] == [M.CELossHead, type(None), M.LabelCELossHead]
    assert tri.wants_groups and not plain.wants_groups and sorted(tri.state_dict()) == sorted(plain.state_dict())


@pytest.mark.parametrize("loss,mode", [("ce_label", {"cat_label": True}), ("ce_val_label", {"text_emb": "clip_text"})])
def test_label_heads_refuse_text_modes_without_labels(loss, mode):
    mon = object.__new__(monitor.VALMonitor)
    mon.cfg = to_config({"eval": False, "model": {"loss": dict(loss_cfg(loss))},
                         "running": dict({"data_root": "/nonexistent", "data_name": "src_train", "audioset_text": True}, **mode)})
    assert monitor.label_positives(mon.cfg) and not monitor.label_positives(to_config({"model": {"loss": dict(loss_cfg("ce_val"))}}))
    with pytest.raises(VipantError, match="label positives"):
        mon.build_audioset_text_data()
    assert not mon.label_groups
