"""Barlow Twins loss groups without a GPU: config groups through the launch-line parser, the reference's module / state-dict
layout (cvap/module/decoder/loss_head.py:287-328, 601-622), construction-time refusals, LARS grouping, the new ABI queries."""
import logging
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VA = ("+running=bimodal worker=CVALP eval=False +model/image=vit_val +model/audio=vit_val +model/text=dummy +optimizer=standard "
      "+running/audio=default")

SMALL_KEYS = ["linear.0.weight", "linear.1.weight", "linear.1.bias", "linear.1.running_mean", "linear.1.running_var",
              "linear.1.num_batches_tracked", "linear.3.weight", "linear.4.weight", "linear.4.bias", "linear.4.running_mean",
              "linear.4.running_var", "linear.4.num_batches_tracked", "linear.6.weight", "bn.running_mean", "bn.running_var",
              "bn.num_batches_tracked"]


def _compose(loss, extra=""):
    from vipant_amd.config import compose
    return compose(f"{VA} +model/loss={loss} {extra}".split())


def test_groups_resolve_through_the_launch_parser():
    sys.path.insert(0, ROOT)
    import train  # noqa: F401  (the entry point's parser is vipant_amd.config.compose)
    b = _compose("barlow").model.loss
    assert dict(b) == {"name": "BarlowLossHead", "embed_dim": 512, "lambd_off": 0.0051, "layers": [2048, 4096, 4096]}
    bc = _compose("barlow_ce", "model.image.embed_dim=256").model.loss
    assert bc.name == "BarlowCELossHead" and bc.lambd_barlow == 0.05 and dict(bc.ce) == {"name": "CELossHead"}
    assert dict(bc.barlow) == {"name": "BarlowLossHead", "embed_dim": 256, "lambd_off": 0.0051, "layers": [2048, 4096, 4096]}


def test_heads_build_on_cpu_with_the_reference_key_set(caplog):
    import vipant_amd.module as M
    head = M.build_loss_head(_compose("barlow").model.loss)
    assert isinstance(head, M.BarlowLossHead) and list(head.state_dict()) == SMALL_KEYS
    assert head.normalized is False and head.reduce is True and head.lambd_off == 0.0051
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert shapes["linear.0.weight"] == (2048, 512) and shapes["linear.3.weight"] == (4096, 2048)
    assert shapes["linear.6.weight"] == (4096, 4096) and shapes["bn.running_var"] == (4096,)
    assert [type(m).__name__ for m in head.linear] == ["Linear", "BatchNorm1d", "ReLU"] * 2 + ["Linear"]
    assert head.bn.affine is False and head.bn.momentum == 0.1 and head.bn.eps == 1e-5
    with caplog.at_level(logging.WARNING):
        bce = M.build_loss_head(_compose("barlow_ce").model.loss)
    assert list(bce.state_dict()) == ["loss_ce.logit_scale"] + ["loss_barlow." + k for k in SMALL_KEYS]
    assert "scaling" in caplog.text and "scale_max" in caplog.text          # the fill of the `ce` sub-config is logged
    assert isinstance(bce.loss_ce.logit_scale, torch.nn.Parameter) and bce.loss_ce.scale_max == float("inf")
    assert bce.lambd_barlow == 0.05
    # a reference-layout state dict loads strictly
    bce.load_state_dict({k: v.clone() for k, v in bce.state_dict().items()}, strict=True)


def test_widths_that_are_not_multiples_of_64_are_refused():
    import vipant_amd.module as M
    from vipant_amd._ffi import VipantError
    cfg = _compose("barlow").model.loss
    cfg.layers = [2048, 4000, 4096]
    with pytest.raises(VipantError, match=r"layers\[1\] = 4000"):
        M.build_loss_head(cfg)
    cfg = _compose("barlow", "model.image.embed_dim=500").model.loss
    with pytest.raises(VipantError, match="embed_dim = 500"):
        M.build_loss_head(cfg)


def test_local_negatives_are_refused():
    import vipant_amd.module as M
    from vipant_amd._ffi import VipantError
    for g in ("barlow", "barlow_ce"):
        with pytest.raises(VipantError, match="negatives='local'"):
            M.build_loss_head(_compose(g).model.loss, negatives="local")


def test_lars_groups_follow_the_ndim_split():
    """Monitor.build_optimizer's two groups (cvap/monitor/cvap.py: ndim > 1 adapted, the rest bias-like): projector weights in the
    first, BN gamma / beta and logit_scale in the second -- no special cases."""
    import vipant_amd.module as M
    bce = M.build_loss_head(_compose("barlow_ce").model.loss)
    params = dict(bce.named_parameters())
    adapted = sorted(k for k, p in params.items() if not M.exclude_bias_or_norm(p))
    assert adapted == ["loss_barlow.linear.0.weight", "loss_barlow.linear.3.weight", "loss_barlow.linear.6.weight"]
    assert sorted(set(params) - set(adapted)) == ["loss_barlow.linear.1.bias", "loss_barlow.linear.1.weight",
                                                  "loss_barlow.linear.4.bias", "loss_barlow.linear.4.weight",
                                                  "loss_ce.logit_scale"]


def test_barlow_workspace_queries_run_without_a_gpu():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    assert _ffi.query("vipant_batchnorm_workspace_bytes", 4096, 4096) == 64 * 4 * 4096 * 4
    assert _ffi.query("vipant_batchnorm_workspace_bytes", 257, 192) == 5 * 4 * 192 * 4
    assert _ffi.query("vipant_barlow_loss_workspace_bytes", 4096) == 64 * 64 * 2 * 4
    assert _ffi.query("vipant_barlow_loss_workspace_bytes", 192) == 3 * 3 * 2 * 4


def test_bad_barlow_arguments_are_reported_not_executed():
    from vipant_amd import _ffi
    with pytest.raises(_ffi.VipantError, match="M >= 2"):
        _ffi.call("vipant_batchnorm_fwd", 16, 64, None, None, 0, 16, 16, 16, None, None, None, 0.1, 1e-5, 1, 64, 16, 1 << 20, None)
    with pytest.raises(_ffi.VipantError, match="workspace"):
        _ffi.call("vipant_batchnorm_bwd", 16, 64, 16, 64, 16, 16, None, None, 0, 16, None, None, 0, 8, 0, 8, 64, None, 0, None)
    with pytest.raises(_ffi.VipantError, match="row range"):
        _ffi.call("vipant_batchnorm_bwd", 16, 64, 16, 64, 16, 16, 16, 16, 0, 16, 16, 16, 4, 8, 0, 8, 64, 16, 1 << 20, None)
    with pytest.raises(_ffi.VipantError, match="go together"):
        _ffi.call("vipant_barlow_loss", 16, 64, 8, 0.0051, 16, None, 16, None, 64, 16, 1 << 20, None)


def test_barlow_head_has_no_cpu_fallback():
    import vipant_amd.module as M
    from vipant_amd._ffi import VipantError
    head = M.build_loss_head(_compose("barlow", "model.loss.layers=[128,256]").model.loss).train()
    with pytest.raises(VipantError, match="no CPU fallback"):
        head(torch.zeros(8, 512), torch.zeros(8, 512), normalized=False)


def test_key_lists_equal_the_reference_fixture():
    """The state-dict key lists recorded from the reference heads (tests/golden/barlow_keys.npz, reference layers)."""
    import numpy as np
    import vipant_amd.module as M
    fx = np.load(os.path.join(ROOT, "tests", "golden", "barlow_keys.npz"))
    assert list(M.build_loss_head(_compose("barlow").model.loss).state_dict()) == list(fx["keys_barlow"])
    assert list(M.build_loss_head(_compose("barlow_ce").model.loss).state_dict()) == list(fx["keys_barlow_ce"])


def test_momentum_none_is_refused():
    """torch's BatchNorm1d(momentum=None) is a cumulative moving average; the kernels implement the exponential one only."""
    import vipant_amd.module as M
    from vipant_amd import ops
    from vipant_amd._ffi import VipantError
    head = M.build_loss_head(_compose("barlow", "model.loss.layers=[128,256]").model.loss)
    head.bn.momentum = None
    with pytest.raises(VipantError, match="momentum=None"):
        ops._bn_state(head.bn)
