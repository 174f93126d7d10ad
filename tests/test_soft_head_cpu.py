"""Host side of the similarity-weighted InfoNCE head: config groups, name resolution, construction-time refusals, `ce_val` without the key."""
import pytest

import vipant_amd.module as M
from vipant_amd._ffi import VipantError
from vipant_amd.config import compose, to_config


def loss_cfg(name, **over):
    return to_config(dict(compose([f"+model/loss={name}"]).model.loss, **over))


def test_groups_compose_and_heads_resolve():
    soft, val, tri = loss_cfg("ce_soft"), loss_cfg("ce_val"), loss_cfg("ce_val_soft")
    assert dict(soft) == {"name": "SoftCELossHead", "layers": [], "scaling": True, "scale_max": None, "teacher": "x2", "w_floor": -1.0, "w_power": 1.0}
    assert {k: (dict(v) if k == "soft_positives" else v) for k, v in dict(tri).items()} == dict(val, w_floor=-1.0, w_power=1.0,
                                                                                             soft_positives={"va": "x1", "al": "x2"})
    head = M.build_loss_head(soft)
    assert type(head) is M.SoftCELossHead is M.MORE_LOSS_HEADS_REGISTRY.get("SoftCELossHead") and issubclass(M.SoftCELossHead, M.CELossHead)
    assert (head.teacher, head.w_floor, head.w_power) == ("x2", -1.0, 1.0) and sorted(head.state_dict()) == ["logit_scale"]
    assert "teacher x2" in head.describe()
    plain, both = M.build_loss_head(val), M.build_loss_head(tri)
    assert "soft_positives" not in val and not hasattr(plain.loss_head_va, "teacher") and plain.describe() == ""
    assert [type(h) for h in (plain.loss_head_va, plain.loss_head_lv, plain.loss_head_al)] == [M.CELossHead, type(None), M.CELossHead]
    assert [type(h) for h in (both.loss_head_va, both.loss_head_lv, both.loss_head_al)] == [M.SoftCELossHead, type(None), M.SoftCELossHead]
    assert (both.loss_head_va.teacher, both.loss_head_al.teacher) == ("x1", "x2") and sorted(both.state_dict()) == sorted(plain.state_dict())


@pytest.mark.parametrize("name,over,word", [("ce_soft", {"w_floor": 1.0}, "w_floor"), ("ce_soft", {"w_floor": -1.5}, "w_floor"),
                                            ("ce_soft", {"w_power": 0.0}, "w_power"), ("ce_soft", {"teacher": "x3"}, "teacher"),
                                            ("ce_val_soft", {"soft_positives": {"vl": "x1"}}, "soft_positives"),
                                            ("ce_val_soft", {"soft_positives": {"va": "given"}}, "soft_positives"),
                                            ("ce_val_soft", {"label_positives": ["al"]}, "both")])
def test_construction_refusals(name, over, word):
    with pytest.raises(VipantError, match=word):
        M.build_loss_head(loss_cfg(name, **over))
