"""Siamese multi-view VA training without a GPU: the config groups compose to the reference's values, the new names resolve
through both package names, the variadic feature all-gather equals per-tensor gathers, the C ABI refuses bad pair graphs."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

OV = ("+running=siamese worker=CVASP monitor=VASMonitor +model/image=vit_val +model/audio=vit_val +model/text=dummy "
      "+model/loss=ce_va +optimizer=standard +running/audio=default model.image.freeze=False")


def test_override_line_composes_to_the_reference_values():
    from vipant_amd.config import compose, to_plain
    cfg = compose(OV.split())
    assert cfg.worker == "CVASP" and cfg.monitor == "VASMonitor" and cfg.model.image.freeze is False
    # configs/model/loss/ce_va.yaml, key for key
    assert to_plain(cfg.model.loss) == dict(name="VACELossHead", layers=[], scaling=True, scale_max=None, vp=True, vp_w=1., ap=False,
                                            ap_w=1., va=True, va_w=1., vv=True, vv_w=1., aa=False, aa_w=1.)
    r = cfg.running                     # configs/running/siamese.yaml (paths default to dataset-free operation)
    assert (r.multi_view, r.batch_size, r.save_rate, r.save_epoch, r.peep_rate, r.eval_samples, r.test_samples, r.epochs) == \
        (True, 432, 300, False, 1, 5184, 5000, 1000)
    assert (r.data_name, r.eval_name, r.test_name, r.clip_tf, r.imagine, r.frame_emb) == \
        ("npz_unbalanced_train_segments", "npz_balanced_train_segments", "eval", False, True, None)
    assert to_plain(r.siamese) == dict(alive=False, keep_hp=True, amodules=[], lmodules=[])
    assert r.resolution == 224 and r.embed_dim == 512 and r.max_audio_len == 1000 and r.num_mel_bins == 128


def test_names_resolve_through_both_packages():
    import cvap.model, cvap.module, cvap.monitor
    import vipant_amd.model, vipant_amd.module, vipant_amd.monitor
    assert cvap.model.CVASP is vipant_amd.model.CVASP is vipant_amd.model.VAL_MODELS_REGISTRY.get("CVASP")
    assert issubclass(cvap.model.CVASP, cvap.model.CVALP)
    assert cvap.monitor.VASMonitor is vipant_amd.monitor.VASMonitor
    assert cvap.module.LOSS_HEADS_REGISTRY.get("VACELossHead") is vipant_amd.module.loss_head.VACELossHead


def _build(extra):
    from vipant_amd.config import compose
    from vipant_amd.model import build_main_model
    cfg = compose((OV + " eval=False model.image.encoder.layers=2 running.clip_model_root=/nonexistent " + extra).split())
    cfg.rank = 0
    lines = []
    model = build_main_model(cfg, lines.append)
    return model, model.build(), lines


def test_state_dict_and_tunable_keys_equal_the_reference(golden):
    """Against tests/golden/vace_keys.npz, made by the reference: the state-dict keys of both head configurations (order included)
    and the names `CVASP._build_siamese_backbone` returns as tunable for `siamese.alive=True amodules=[encoder]`, image tower
    frozen and trainable."""
    g = golden("vace_keys")
    model, tunable, _ = _build("model.loss.ap=True model.loss.aa=True")
    assert list(model.loss_head.state_dict()) == [str(k) for k in g["keys_vace_all"]]
    model, tunable, _ = _build("")
    assert list(model.loss_head.state_dict()) == [str(k) for k in g["keys_vace_default"]]
    assert any(k.startswith("image_head.encoder.") for k in tunable) and any(k.startswith("audio_head.encoder.") for k in tunable)
    shared = "running.siamese.alive=True running.siamese.amodules=[encoder] "
    model, tunable, lines = _build(shared + "model.image.freeze=True")
    assert model.audio_head.encoder is model.image_head.encoder
    assert set(tunable) == {str(k) for k in g["tunable_shared_frozen_image"]} and len(tunable) == len(g["tunable_shared_frozen_image"])
    assert any("Freeze image encoder (excl. shared modules: {'encoder'})" in l for l in lines)
    # what the fixture says, spelled out: the shared blocks under the image head's names, nothing else of the image tower
    img = {k for k in tunable if k.startswith("image_head.")}
    assert img and all(k.startswith("image_head.encoder.") for k in img) and not any(k.startswith("audio_head.encoder.") for k in tunable)
    model, tunable, _ = _build(shared + "model.image.freeze=False")
    assert set(tunable) == {str(k) for k in g["tunable_shared_trainable_image"]} and len(tunable) == len(g["tunable_shared_trainable_image"])


def test_a_disabled_pair_has_no_sub_head():
    model, tunable, _ = _build("model.loss.vv=False")
    assert list(model.loss_head.state_dict()) == ["loss_head_vp.logit_scale", "loss_head_va.logit_scale"]
    assert model.loss_head.loss_head_vv is None and list(model.loss_head._total_loss) == ["vp", "va"]


def _gather_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vipant_amd import parallel
        g = torch.Generator().manual_seed(100 + rank)
        xs = [torch.randn(3, 8, generator=g).requires_grad_() for _ in range(4)]
        calls = []
        orig = parallel._AllGatherRows.apply
        parallel._AllGatherRows.apply = staticmethod(lambda x: (calls.append(1), orig(x))[1])
        packed = parallel.all_gather_features(*xs)
        pair = parallel.all_gather_features(xs[0], xs[1])
        parallel._AllGatherRows.apply = orig
        single = [parallel._AllGatherRows.apply(x) for x in xs]
        ok = len(calls) == 2 and len(packed) == 4 and len(pair) == 2
        ok = ok and all(torch.equal(a, b) and a.is_contiguous() for a, b in zip(packed, single))
        ok = ok and torch.equal(pair[0], single[0]) and torch.equal(pair[1], single[1])
        sum((i + 1) * p.sum() for i, p in enumerate(packed)).backward()          # the backward keeps this rank's rows
        ok = ok and all(torch.equal(x.grad, torch.full_like(x, float(i + 1))) for i, x in enumerate(xs))
        out[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


def test_variadic_all_gather_equals_per_tensor_gathers():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_gather_worker, args=(2, port, out), nprocs=2, join=True)
    assert dict(out) == {0: True, 1: True}


def test_binding_declares_the_entry_point_and_its_refusals():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    assert len(_ffi.PROTOTYPES["vipant_infonce_multi_fwd_bwd"][1]) == 19
    assert _ffi.query("vipant_infonce_multi_workspace_bytes", 432, 512, 4, 3, 432) > 3 * 2 * 432 * 512 * 4
    assert _ffi.query("vipant_infonce_multi_workspace_bytes", 432, 512, 6, 3, 432) == 0

    def call(pairs, nop=3, E=512, dx=(None, None, None)):
        n = len(pairs)
        _ffi.call("vipant_infonce_multi_fwd_bwd", (C.c_void_p * nop)(*[16] * nop), nop, (C.c_int32 * n)(*[a for a, _ in pairs]),
                  (C.c_int32 * n)(*[b for _, b in pairs]), n, 16, (C.c_float * n)(), (C.c_float * n)(*[1.0] * n), 16,
                  (C.c_void_p * nop)(*dx), None, 1.0, 64, E, 0, 64, None, 0, None)
    for kwargs, msg in ((dict(pairs=[(0, 0)]), "against itself"), (dict(pairs=[(0, 3)]), "out of range"),
                        (dict(pairs=[(0, 1)], E=480), "E % 64"), (dict(pairs=[(0, 1)], dx=(None, None, 16)), "in no pair"),
                        (dict(pairs=[(0, 1)] * 6), "1 to 5"), (dict(pairs=[(0, 1)]), "workspace too small")):
        with pytest.raises(_ffi.VipantError, match=re.escape(msg)):
            call(**kwargs)
