"""The classification path against the REFERENCE's own outputs (tests/golden/make_golden_cls.py): the ESClassifier glue end to
end, the supervised p1 report, and the zero-shot report through ClassificationHead.report(text=...).

Budgets: `e2e_cls` loss within 1e-3, features and tower gradients under the end-to-end rule of test_barlow_golden_gpu.py
(features 2 % of scale; on the five tensors that test checks, the norm within 5 % and rel-L2 of the sampled entries within 0.15).
The supervised p1 string is compared on the samples whose reference top-2 logit gap is at least 4 x the largest logit error of a
bf16-operand emulation of the reference head (computed here, in float64); at most 2 % of the samples may be left out."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen  # noqa: E402  (tests/golden on sys.path via conftest)
import gen_cls  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LINE = ("+running=esc50 worker=ESClassifier monitor=ESCMonitor +model/audio=vit_val +model/image=vit_val "
        "+model/text=transformer_val +model/loss=ce_cls +optimizer=standard +running/audio=default")


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30))


def _head(tag, C):
    import vipant_amd.module as M
    from vipant_amd.config import to_config
    head = M.build_loss_head(to_config({"name": "ClassificationHead", "embed_dim": 512, "layers": [], "scaling": True}), output_dim=C)
    head.load_state_dict(dict(head.state_dict(), **gen_cls.head_weights(tag, head.state_dict(), C)), strict=True)
    return head


def test_e2e_esclassifier_against_reference(golden):
    from vipant_amd.config import compose
    from vipant_amd.model import ESClassifier
    fx = golden("e2e_cls")
    tag, L, b, T_, Fq, C = "e2e_cls", 2, 32, 256, 64, 50
    cfg = compose((f"{LINE} eval=False num_gpus=1 model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers={L} "
                   f"running.audio.max_len={T_} running.audio.num_mel_bins={Fq} running.batch_size={b} "
                   "running.clip_model_root=/nonexistent").split())
    model = ESClassifier(cfg, lambda *_: None)
    tunable = model.build(output_dim=C)
    assert any(k.startswith("audio_head.") for k in tunable) and "loss_head.logit_scale" in tunable
    S = model.audio_head.misc.positional_embedding.shape[0]
    assert S == int(fx["S"])
    model.audio_head.load_state_dict({k: v.to(DEV) for k, v in gen.det_weights(f"{tag}/audio", gen.vit_head_shapes(768, L, 512, S)).items()},
                                     strict=True)
    lh = model.loss_head
    lh.load_state_dict(dict(lh.state_dict(), **{k: v.to(DEV) for k, v in gen_cls.head_weights(tag, lh.state_dict(), C, gain=gen_cls.E2E_GAIN).items()}), strict=True)
    model.train()
    aud = gen.det_randn(f"{tag}/aud", (b, 1, T_, Fq))
    assert np.allclose(gen.checksum(aud), fx["aud_sum"])
    labels = (torch.arange(b) * 7) % C
    feats = {}
    model.audio_head.register_forward_hook(lambda m, i, o: feats.__setitem__("a", o))
    loss = model(aud.to(DEV), labels.to(DEV))
    loss.backward()
    feat = feats["a"].detach().double().cpu()
    want = torch.from_numpy(fx["feat"]).double()
    ferr = float((feat - want).abs().max() / want.abs().max())
    lerr = abs(float(loss) - float(fx["loss"]))
    print(f"[e2e_cls] loss hip={float(loss):.6f} reference={float(fx['loss']):.6f} diff {lerr:.2e}; feature err {ferr:.2e}")
    assert ferr < 2e-2, ferr
    assert lerr <= 1e-3, (float(loss), float(fx["loss"]))
    for k, p in lh.named_parameters():
        e = _rel(p.grad.detach().cpu().numpy(), fx[f"g_{k}"])
        print(f"[e2e_cls] head gradient {k}: rel-L2 {e:.2e}")
        assert e < 0.15, (k, e)
    checked = ("misc.class_embedding", "misc.positional_embedding", "post_encoder.proj", "pre_encoder.conv1.weight",
               "encoder.resblocks.0.attn.in_proj_bias")
    errs, norms = {}, {}
    for k, p in model.audio_head.named_parameters():
        g = p.grad.detach().double().cpu().reshape(-1)
        idx = torch.from_numpy(fx[f"t_idx_{k}"])
        errs[k] = _rel(g[idx].numpy(), fx[f"t_s_{k}"])
        r = float((g * g).sum()) / float(fx[f"t_sum_{k}"][1])
        norms[k] = r ** 0.5
        if k in checked:
            assert abs(r ** 0.5 - 1) < 5e-2, (k, r ** 0.5)
            assert errs[k] < 0.15, (k, errs[k])
    print("[e2e_cls] audio-tower gradients (rel-L2 of the sampled entries, norm ratio): "
          + ", ".join(f"{k}=({v:.2e}, {norms[k]:.3f})" for k, v in errs.items()))


@pytest.mark.parametrize("tag", ["cls_esc50", "cls_us8k"])
def test_supervised_p1_report(golden, tag):
    fx = golden("cls_reports")
    kind, B, C, layers, bias, scaling, n = gen_cls.CASES[tag]
    head = _head(tag, C)
    x, y = gen_cls.ce_inputs(tag, n, C, part=gen_cls.EVAL_PART[tag])
    # float64 reference logits and their bf16-operand emulation (LayerNorm output and weight rounded)
    ln, lin = head.linear[0], head.linear[1]
    h = F.layer_norm(x.double(), (512,), ln.weight.double(), ln.bias.double(), 1e-5)
    scale = float(head.logit_scale.detach().exp())
    exact = scale * (h @ lin.weight.double().t() + lin.bias.double())
    r = lambda t: t.to(torch.bfloat16).double()
    emu = scale * (r(h) @ r(lin.weight.detach().double()).t() + lin.bias.double())
    err = float((exact - emu).abs().max())
    top2 = exact.topk(2, dim=-1)[0]
    keep = (top2[:, 0] - top2[:, 1]) >= 4 * err
    left_out = int((~keep).sum())
    print(f"[{tag}] bf16-emulation logit error {err:.4f}, margin {4 * err:.3f} leaves out {left_out} of {n}")
    assert left_out <= 0.02 * n, (left_out, n)
    want = str(fx[f"report_{tag}"])
    assert want == f"A->T: p1 = {(exact.argmax(-1) == y).sum() / n * 100.:2.2f} @ {n}", "the restatement is not the reference"
    head = head.to(DEV).eval()
    with torch.no_grad():
        for i in range(0, n, 100):
            assert head(x[i:i + 100].to(DEV), y[i:i + 100].to(DEV), names=[f"s{j}" for j in range(i, i + 100)]) is None
    pred = torch.cat(head.x1s).cpu()
    assert len(head.ids) == n and torch.cat(head.audios).shape == (n, 512)
    assert torch.equal(pred[keep], exact.argmax(-1)[keep]), int((pred[keep] != exact.argmax(-1)[keep]).sum())
    report = head.report()
    print(f"[{tag}] hip `{report}` reference `{want}`")
    if left_out == 0:
        assert report == want
    else:       # the samples left out may move the precision by their share at most
        got = float(report.split("=")[1].split("@")[0])
        assert abs(got - float(want.split("=")[1].split("@")[0])) <= 100.0 * left_out / n + 0.005 and report.endswith(f"@ {n}")
    assert not hasattr(head, "x1s")


def test_zero_shot_report_through_the_head(golden):
    """ClassificationHead.report(text=...) with and without `label_map` equals the strings make_golden.py records."""
    fx = golden("report_protocols")
    import vipant_amd.module as M
    from vipant_amd.config import to_config
    head = M.build_loss_head(to_config({"name": "ClassificationHead", "embed_dim": 512, "layers": [], "scaling": True}),
                             output_dim=50).to(DEV).eval()
    prompts = gen.det_randn("zs/text", (50, 512)); prompts = prompts / prompts.norm(dim=-1, keepdim=True)
    lab = (torch.arange(200) * 7) % 50
    feats = prompts[lab] + 7.0 * gen.det_randn("zs/noise", (200, 512)) / 512 ** 0.5
    feats = feats / feats.norm(dim=-1, keepdim=True)
    with torch.no_grad():
        head(feats[:120].to(DEV), lab[:120].to(DEV)); head(feats[120:].to(DEV), lab[120:].to(DEV))
        assert head.report(text=prompts.to(DEV)) == str(fx["zero_shot"])
        perm = {i: (i * 3) % 50 for i in range(50)}
        mapped = torch.tensor([perm[int(v)] for v in lab])
        head(feats[:120].to(DEV), mapped[:120].to(DEV)); head(feats[120:].to(DEV), mapped[120:].to(DEV))
        assert head.report(text=prompts.to(DEV), label_map=perm) == str(fx["zero_shot_mapped"])
