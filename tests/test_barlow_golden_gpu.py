"""Barlow Twins heads against the REFERENCE's own outputs (tests/golden/make_golden_barlow.py ran cvap's BarlowLossHead /
BarlowCELossHead and the CVALP VA glue on the same generated weights and inputs).

Budgets (the issue's): loss within 1e-3 relative; every gradient and running statistic within 1.5 x the distance of a CPU
bf16-operand emulation (test_barlow_gpu.ref_barlow, emulate=True) from the same reference output, + 1e-3 (gradients) / + 1e-5
(running statistics).  The test's float64 restatement itself (emulate=False) must sit within fp32 rounding of the reference: loss, parts and running
statistics to 1e-5, gradients to 5e-3 (the fp32 reference program's own error: at the reference widths its rounding moves a few
pre-activations across ReLU's kink, 1.6e-3 observed on dW0).  That pins the restatement -- two running-statistics updates per
step, BN placement, the 1 / B scaling -- to the reference program.
Weight gradients are stored as 4096 seeded entries + (sum, sum of squares); the rest in full."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen  # noqa: E402  (tests/golden on sys.path via conftest)
import make_golden_barlow as MGB  # noqa: E402  (weight / input generators only; nothing of the reference is imported)
import test_barlow_gpu as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAMBD = 0.0051


def _load(golden, name):
    g = golden(name)
    return {k: g[k] for k in g.files}


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def _compare(fx, name, got, emu, ref64, what, floor=1e-3, restate_tol=5e-3):
    """got / emu / ref64: full tensors of one quantity; fx holds g_<name> (full) or idx_ / s_ / sum_<name> (samples)."""
    got, emu, ref64 = (t.detach().double().cpu().reshape(-1) for t in (got, emu, ref64))
    if f"g_{name}" in fx:
        want = fx[f"g_{name}"]
        pick = lambda t: t.numpy()
    else:
        idx = torch.from_numpy(fx[f"idx_{name}"])
        want = fx[f"s_{name}"]
        pick = lambda t: t[idx].numpy()
        ssq = float(fx[f"sum_{name}"][1])
        assert abs(float((got * got).sum()) / ssq - 1) <= 1.5 * abs(float((emu * emu).sum()) / ssq - 1) + 2 * floor, (what, name)
    e_hip, e_emu, e_64 = _rel(pick(got), want), _rel(pick(emu), want), _rel(pick(ref64), want)
    assert e_64 <= restate_tol, (what, name, "float64 restatement vs reference", e_64)
    assert e_hip <= 1.5 * e_emu + floor, (what, name, e_hip, e_emu)
    return e_hip, e_emu


def _barlow_head(tag, layers):
    import vipant_amd.module as M
    head = M.build_loss_head(T._barlow_cfg(layers))
    head.load_state_dict(dict(head.state_dict(), **MGB.barlow_weights(tag, head)), strict=True)
    return head


@pytest.mark.parametrize("tag", ["barlow_small", "barlow_default"])
def test_barlow_head_against_reference(golden, tag):
    fx = _load(golden, tag)
    B, layers = int(fx["B"]), [int(w) for w in fx["layers"]]
    head = _barlow_head(tag, layers)
    assert list(head.state_dict()) == list(fx["keys"])
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    x1, x2 = MGB.inputs(tag, B)
    head = head.to(DEV).train()
    x1d, x2d = x1.to(DEV).requires_grad_(), x2.to(DEV).requires_grad_()
    loss = head(x1d, x2d, normalized=False)
    loss.backward()
    L = len(layers) - 1
    ref = T.ref_barlow(sd, L, x1, x2, LAMBD, emulate=False)
    emu = T.ref_barlow(sd, L, x1, x2, LAMBD, emulate=True)
    for r in (ref, emu):
        r[0].backward()
    assert abs(float(loss) / float(fx["loss"]) - 1) <= 1e-3, (float(loss), float(fx["loss"]))
    assert abs(float(ref[0]) / float(fx["loss"]) - 1) <= 1e-5
    parts = head.parts.cpu().double()
    for i, k in ((1, "on"), (2, "off")):
        want = float(fx[k])
        assert abs(float(ref[i]) / want - 1) <= 1e-5, k
        assert abs(float(parts[i]) - want) <= 1.5 * abs(float(emu[i]) - want) + 1e-3 * want, (k, float(parts[i]), want)
    out = {}
    params = dict(head.named_parameters())
    for k in ref[3]:
        out[k] = _compare(fx, k, params[k].grad, emu[3][k].grad, ref[3][k].grad, tag)
    out["dx1"] = _compare(fx, "dx1", x1d.grad, emu[5].grad, ref[5].grad, tag)
    out["dx2"] = _compare(fx, "dx2", x2d.grad, emu[6].grad, ref[6].grad, tag)
    bufs = dict(head.named_buffers())
    for k in emu[4]:
        want = fx[f"buf_{k}"]
        e_hip, e_emu, e_64 = _rel(bufs[k].cpu(), want), _rel(emu[4][k], want), _rel(ref[4][k], want)
        assert e_64 <= 1e-5, (k, e_64)
        assert e_hip <= 1.5 * e_emu + 1e-5, (k, e_hip, e_emu)
        out[k] = (e_hip, e_emu)
    for k, v in bufs.items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == int(fx[f"buf_{k}"]) == 2, k
    print(f"[{tag}] loss hip={float(loss):.6f} reference={float(fx['loss']):.6f}; rel err vs reference (hip, bf16-emulation): "
          + ", ".join(f"{k}=({a:.3e}, {b:.3e})" for k, (a, b) in out.items()))


def test_barlow_ce_head_against_reference(golden):
    import vipant_amd.module as M
    fx = _load(golden, "barlow_ce")
    B, layers = int(fx["B"]), [int(w) for w in fx["layers"]]
    from vipant_amd.config import to_config
    head = M.build_loss_head(to_config({"name": "BarlowCELossHead", "lambd_barlow": 0.05, "ce": {"name": "CELossHead"},
                                        "barlow": dict(T._barlow_cfg(layers))}))
    w = {"loss_barlow." + k: v for k, v in MGB.barlow_weights("barlow_ce", head.loss_barlow).items()}
    head.load_state_dict(dict(head.state_dict(), **w), strict=True)
    assert list(head.state_dict()) == list(fx["keys"])
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    x1, x2 = MGB.inputs("barlow_ce", B)
    head = head.to(DEV).train()
    x2d = x2.to(DEV).requires_grad_()
    loss = head(x1.to(DEV), x2d, normalized=False)
    loss.backward()
    bsd = {k[len("loss_barlow."):]: v for k, v in sd.items() if k.startswith("loss_barlow.")}
    runs = {}
    for emulate in (False, True):
        lb, on, off, P, R, r1, r2 = T.ref_barlow(bsd, len(layers) - 1, x1, x2, LAMBD, emulate)
        ls = sd["loss_ce.logit_scale"].double().clone().requires_grad_()
        a, b = F.normalize(r1, dim=-1), F.normalize(r2, dim=-1)
        logits = ls.exp() * a @ b.t()
        lab = torch.arange(B)
        lce = F.cross_entropy(logits, lab) + F.cross_entropy(logits.t(), lab)
        (lce + 0.05 * lb).backward()
        runs[emulate] = (lce + 0.05 * lb, lce, P, ls, r2, R)
    ref, emu = runs[False], runs[True]
    assert abs(float(loss) / float(fx["loss"]) - 1) <= 1e-3, (float(loss), float(fx["loss"]))
    # (the InfoNCE part is ~4e-4 of a ~2.2 loss here: its fp32 reference value is held to 1e-5 of the total, not of itself)
    assert abs(float(ref[0]) / float(fx["loss"]) - 1) <= 1e-5
    assert abs(float(ref[1]) - float(fx["loss_ce"])) <= 1e-5 * float(fx["loss"])
    params = dict(head.named_parameters())
    _compare(fx, "loss_ce.logit_scale", params["loss_ce.logit_scale"].grad, emu[3].grad, ref[3].grad, "barlow_ce")
    for k in ref[2]:
        _compare(fx, "loss_barlow." + k, params["loss_barlow." + k].grad, emu[2][k].grad, ref[2][k].grad, "barlow_ce")
    _compare(fx, "dx2", x2d.grad, emu[4].grad, ref[4].grad, "barlow_ce")
    bufs = dict(head.named_buffers())
    for k in ref[5]:
        want = fx[f"buf_loss_barlow.{k}"]
        assert _rel(ref[5][k], want) <= 1e-5, k
        assert _rel(bufs["loss_barlow." + k].cpu(), want) <= 1.5 * _rel(emu[5][k], want) + 1e-5, k


def test_state_dict_keys_and_eval_reports_equal_the_reference(golden):
    import vipant_amd.module as M
    from vipant_amd.config import to_config
    fx = _load(golden, "barlow_keys")
    bar = M.build_loss_head(T._barlow_cfg([2048, 4096, 4096]))
    bce = M.build_loss_head(to_config({"name": "BarlowCELossHead", "lambd_barlow": 0.05, "ce": {"name": "CELossHead"},
                                       "barlow": dict(T._barlow_cfg([2048, 4096, 4096]))}))
    assert list(bar.state_dict()) == list(fx["keys_barlow"])
    assert list(bce.state_dict()) == list(fx["keys_barlow_ce"])
    small = M.build_loss_head(T._barlow_cfg([256, 512, 512]))
    x1, x2 = MGB.inputs("barlow_report", 96)
    for h, want in ((small, fx["report_barlow"]), (bce, fx["report_barlow_ce"])):
        h = h.to(DEV).eval()
        with torch.no_grad():
            for i in range(0, 96, 32):
                h(x1[i:i + 32].to(DEV), x2[i:i + 32].to(DEV), normalized=False)
        assert h.report() == str(want)


def test_e2e_cvalp_barlow_ce_against_reference(golden):
    """CVALP built from `+model/loss=barlow_ce` (VA layout, pre-computed image features): loss, audio features and audio-tower
    gradients against the reference's VA glue (cvalp.py:34-62) on the same weights and inputs."""
    from vipant_amd.config import compose
    from vipant_amd.model.cvalp import CVALP
    fx = _load(golden, "e2e_barlow_ce")
    tag, L, b, T_, Fq = "e2e_barlow_ce", 2, 32, 256, 64
    cfg = compose(("+running=bimodal worker=CVALP eval=False num_gpus=1 +model/image=vit_val +model/audio=vit_val "
                   "+model/text=dummy +model/loss=barlow_ce +optimizer=standard +running/audio=default "
                   f"model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers={L} running.audio.max_len={T_} "
                   f"running.audio.num_mel_bins={Fq} running.frame_emb=synthetic running.batch_size={b}").split())
    model = CVALP(cfg, lambda *_: None)
    model.build()
    assert model.image_head is None and model.text_head is None
    S = model.audio_head.misc.positional_embedding.shape[0]
    assert S == int(fx["S"])
    model.audio_head.load_state_dict({k: v.to(DEV) for k, v in gen.det_weights(f"{tag}/audio", gen.vit_head_shapes(768, L, 512, S)).items()},
                                     strict=True)
    lh = model.loss_head
    w = {"loss_barlow." + k: v.to(DEV) for k, v in MGB.barlow_weights(tag, lh.loss_barlow).items()}
    lh.load_state_dict(dict(lh.state_dict(), **w), strict=True)
    model.train()
    aud = gen.det_randn(f"{tag}/aud", (b, 1, T_, Fq))
    assert np.allclose(gen.checksum(aud), fx["aud_sum"])
    img = gen.det_randn(f"{tag}/img", (b, 512))
    feats = {}
    model.audio_head.register_forward_hook(lambda m, i, o: feats.__setitem__("a", o))
    loss = model(img.to(DEV), aud.to(DEV), None)
    loss.backward()
    feat = feats["a"].detach().double().cpu()
    want = torch.from_numpy(fx["feat"]).double()
    # the project's end-to-end budgets through bf16 towers (tests/test_model_gpu.py: features 2 % of scale, gradients 5 % rel-L2)
    ferr = float((feat - want).abs().max() / want.abs().max())
    lerr = abs(float(loss) / float(fx["loss"]) - 1)
    print(f"[e2e_barlow_ce] loss hip={float(loss):.6f} reference={float(fx['loss']):.6f} rel {lerr:.2e}; feature err {ferr:.2e}")
    assert ferr < 2e-2, ferr
    assert lerr <= 1e-3, (float(loss), float(fx["loss"]))
    # gradients: on the five tensors the project's InfoNCE end-to-end test checks entry by entry, the norm within 5 % (its budget)
    # and rel-L2 on the sampled entries within 0.15.  A gradient that is a column sum of the feature gradient (post_encoder.ln.bias)
    # is not bounded: the head's BatchNorm makes the Barlow term's column sums cancel exactly in the reference, and the bf16 BN
    # backward leaves that cancelled term at bf16 noise (its norm reads 1.14 x the reference's).  Looser than its 5 % by construction: the
    # Barlow head hands the tower a feature gradient that is already 3.6e-2 rel-L2 from the reference's -- the bf16-operand
    # emulation's own distance (test_barlow_head_against_reference) -- where the InfoNCE head's is ~1e-3; the tower's bf16 noise
    # comes on top (0.11 observed on block 0's in_proj_bias).  The other tensors are reported.
    checked = ("misc.class_embedding", "misc.positional_embedding", "post_encoder.proj", "pre_encoder.conv1.weight",
               "encoder.resblocks.0.attn.in_proj_bias")
    errs, norms = {}, {}
    for k, p in model.audio_head.named_parameters():
        g = p.grad.detach().double().cpu().reshape(-1)
        idx = torch.from_numpy(fx[f"idx_{k}"])
        errs[k] = _rel(g[idx].numpy(), fx[f"s_{k}"])
        r = float((g * g).sum()) / float(fx[f"sum_{k}"][1])
        norms[k] = r ** 0.5
        if k in checked:
            assert abs(r ** 0.5 - 1) < 5e-2, (k, r ** 0.5)
            assert errs[k] < 0.15, (k, errs[k])
    print("[e2e_barlow_ce] audio-tower gradients (rel-L2 of the sampled entries, norm ratio): "
          + ", ".join(f"{k}=({v:.2e}, {norms[k]:.3f})" for k, v in errs.items()))
