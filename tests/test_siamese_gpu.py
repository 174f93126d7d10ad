"""VACELossHead, CVASP and VASMonitor on the MI355X.

The loss head against the fp64 restatement of tests/test_infonce_multi_gpu.py (loss within 1e-3 per pair and in total, the
project's loss budget; gradients by the bf16-emulation rule of that file) and against the same terms composed from CELossHead
calls; the worker's one-batch image pass against two passes; four trainer steps on the synthetic five-slot loader."""
import re
from types import SimpleNamespace as NS

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_infonce_multi_gpu import errs, reference  # noqa: E402  (tests/ on sys.path via conftest)

DEV = "cuda:0"
OV = ("+running=siamese worker=CVASP monitor=VASMonitor +model/image=vit_val +model/audio=vit_val +model/text=dummy "
      "+model/loss=ce_va +optimizer=standard +running/audio=default num_gpus=1 eval=False model.image.freeze=False "
      "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=2 running.audio.max_len=256 running.audio.num_mel_bins=64 "
      "running.batch_size=4 running.synthetic_steps=4 optimizer.epochs=1 optimizer.warmup_epoch=1 running.clip_model_root=/nonexistent")


def loss_cfg(**over):
    cfg = dict(name="VACELossHead", layers=[], scaling=True, scale_max=None, vp=True, vp_w=1., ap=False, ap_w=1., va=True, va_w=1.,
               vv=True, vv_w=1., aa=False, aa_w=1.)
    cfg.update(over)
    return NS(**cfg)


def features(B, n, seed):
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    base = torch.randn(B, 512, generator=g)
    return [(base + 3.0 * torch.randn(B, 512, generator=g)).to(DEV) for _ in range(n)]


@pytest.mark.parametrize("B,over,scales", [
    (48, {}, {"vp": 2.0, "va": 2.6593, "vv": 3.1}),
    (130, dict(ap=True, aa=True, vp_w=1., ap_w=.5, va_w=2., vv_w=.25, aa_w=1.5, scale_max=18.0),
     {"vp": 2.0, "ap": 2.3, "va": 2.6593, "vv": 3.1, "aa": 2.5})])        # exp(3.1) = 22.2 > 18: the clamp is active on exactly one pair
def test_head_against_fp64_and_composed_heads(B, over, scales):
    from vipant_amd import module as M
    head = M.build_loss_head(loss_cfg(**over)).to(DEV).train()
    assert sorted(head.state_dict()) == sorted(f"loss_head_{k}.logit_scale" for k in scales)
    with torch.no_grad():
        for k, v in scales.items():
            getattr(head, f"loss_head_{k}").logit_scale.fill_(v)
    prime, v1, a1, v2, a2 = features(B, 5, B)
    for t in (v1, a1, v2, a2):
        t.requires_grad_()
    live_aa = bool(over.get("aa", False))
    loss = head(prime, v1, a1, images_v2=v2, audios_v2=a2 if live_aa else None, normalized=False)
    loss.backward()
    # fp64 on the normalised operands, chained through the normalisation by autograd
    names = ["prime", "v1", "a1", "v2"] + (["a2"] if live_aa else [])
    raw = dict(prime=prime, v1=v1, a1=a1, v2=v2, a2=a2)
    order = [("vp", "v1", "prime"), ("ap", "a1", "prime"), ("va", "v1", "a1"), ("vv", "v1", "v2"), ("aa", "a1", "a2")]
    livep = [(k, a, b) for k, a, b in order if k in scales]
    xs64 = [raw[n].detach().double().requires_grad_() for n in names]
    xn = [x / x.norm(dim=-1, keepdim=True) for x in xs64]
    pairs = [(names.index(a), names.index(b)) for _, a, b in livep]
    ls = [scales[k] for k, _, _ in livep]
    smax = [float(over.get("scale_max") or 0.0)] * len(pairs)
    wts = [float(getattr(head, f"{k}_w")) for k, _, _ in livep]
    losses, total, dxn, emun, dls = reference([x.detach().float() for x in xn], pairs, ls, smax, wts, 1.0)
    for k, (key, _, _) in enumerate(livep):
        got = float(head._total_loss[key])
        print(f"[vace B={B}] {key}: hip={got:.6f} fp64={losses[k]:.6f}")
        assert abs(got - losses[k]) <= 1e-3
        g = float(getattr(head, f"loss_head_{key}").logit_scale.grad)
        if smax[k] > 0 and ls[k] > 2.89:
            assert g == 0.0
        else:
            assert abs(g - dls[k]) <= 1e-4 + 1e-3 * abs(dls[k]), (key, g, dls[k])
    assert abs(float(loss) - total) <= 1e-3
    for i, n in enumerate(names[1:], start=1):
        ref, = torch.autograd.grad(xn[i], xs64[i], dxn[i], retain_graph=True)
        emu, = torch.autograd.grad(xn[i], xs64[i], emun[i], retain_graph=True)
        (hl2, hmx), (el2, emx) = errs(raw[n].grad, ref), errs(emu, ref)
        print(f"    d{n}: rel L2 hip={hl2:.3e} emu={el2:.3e}; max-abs hip={hmx:.3e} emu={emx:.3e}")
        assert hl2 <= 1.5 * el2 + 1e-3 and hmx <= 1.5 * emx + 1e-3, (n, hl2, el2, hmx, emx)
    # the same terms composed from CELossHead calls: every per-pair loss bit for bit
    for k, (key, a, b) in enumerate(livep):
        sub = getattr(head, f"loss_head_{key}")
        term = sub(raw[a].detach(), raw[b].detach(), normalized=False)
        assert float(term) == float(head._total_loss[key]), key
    # stats: the reference's format, running means over nstep
    assert re.fullmatch(" ".join(rf"{k} \d+\.\d{{3}}" for k, _, _ in livep), head.stats(nstep=1)), head.stats(nstep=1)


@pytest.mark.parametrize("tag", ["vace_default", "vace_all"])
def test_head_matches_the_reference_fixtures(golden, tag):
    """Loss within 1e-3 per pair and in total (the project's loss budget); gradients within 1.5 x the error of the bf16-operand
    emulation + 1e-3, the emulation's error computed here in fp64 on the same inputs; d logit_scale as in test_infonce_golden."""
    import gen_siamese as G
    from vipant_amd import module as M
    g = golden(tag)
    B, over = G.CASES[tag]
    head = M.build_loss_head(G.loss_cfg(**over)).to(DEV).train()
    G.set_scales(head)
    raw = dict(zip(("prime", "v1", "a1", "v2", "a2"), (t.to(DEV) for t in G.vace_inputs(tag, B))))
    for n in ("v1", "a1", "v2", "a2"):
        raw[n].requires_grad_()
    loss = head(raw["prime"], raw["v1"], raw["a1"], images_v2=raw["v2"], audios_v2=raw["a2"], normalized=False)
    loss.backward()
    print(f"[{tag}] loss hip={float(loss):.6f} reference={float(g['loss']):.6f}")
    assert abs(float(loss) - float(g["loss"])) <= 1e-3
    order = [("vp", "v1", "prime"), ("ap", "a1", "prime"), ("va", "v1", "a1"), ("vv", "v1", "v2"), ("aa", "a1", "a2")]
    livep = [(k, a, b) for k, a, b in order if k in head._total_loss]
    for key, _, _ in livep:
        assert abs(float(head._total_loss[key]) - float(g[f"loss_{key}"])) <= 1e-3, key
        got, ref = float(getattr(head, f"loss_head_{key}").logit_scale.grad), float(g[f"dls_{key}"])
        assert abs(got - ref) <= 1e-4 + 1e-3 * abs(ref), (key, got, ref)
    names = ["prime", "v1", "a1", "v2"] + (["a2"] if "aa" in head._total_loss else [])
    xs64 = [raw[n].detach().double().requires_grad_() for n in names]
    xn = [x / x.norm(dim=-1, keepdim=True) for x in xs64]
    smax = float(over.get("scale_max") or 0.0)
    _, _, dxn, emun, _ = reference([x.detach().float() for x in xn], [(names.index(a), names.index(b)) for _, a, b in livep],
                                   [G.SCALES[k] for k, _, _ in livep], [smax] * len(livep),
                                   [float(getattr(head, f"{k}_w")) for k, _, _ in livep], 1.0)
    for i, n in enumerate(names[1:], start=1):
        ref = torch.from_numpy(g[f"d{n}"]).to(DEV)
        exact, = torch.autograd.grad(xn[i], xs64[i], dxn[i], retain_graph=True)
        emu, = torch.autograd.grad(xn[i], xs64[i], emun[i], retain_graph=True)
        (hl2, hmx), (el2, emx) = errs(raw[n].grad, ref), errs(emu, exact)
        print(f"    d{n}: rel L2 hip={hl2:.3e} emu={el2:.3e}; max-abs hip={hmx:.3e} emu={emx:.3e}")
        assert hl2 <= 1.5 * el2 + 1e-3 and hmx <= 1.5 * emx + 1e-3, (n, hl2, el2, hmx, emx)
    if "aa" not in head._total_loss:
        assert raw["a2"].grad is None


def test_keys_stats_and_report_strings_equal_the_reference(golden):
    import gen_siamese as G
    from vipant_amd import module as M
    g = golden("vace_keys")
    for tag, (_, over) in G.CASES.items():
        assert list(M.build_loss_head(G.loss_cfg(**over)).state_dict()) == [str(k) for k in g[f"keys_{tag}"]]
    head = M.build_loss_head(G.loss_cfg()).to(DEV).train()
    G.set_scales(head)
    for step in range(2):
        prime, v1, a1, v2, a2 = (t.to(DEV) for t in G.vace_inputs(f"vace_stats/{int(g['stats_seed'])}/{step}", 48))
        head(prime, v1, a1, images_v2=v2, audios_v2=a2, normalized=False)
    assert head.stats(nstep=2) == str(g["stats"])
    head.eval()
    ops5 = [t.to(DEV) for t in G.vace_inputs("vace_report", 200, noise=0.3)]
    with torch.no_grad():
        for i in (0, 100):
            prime, v1, a1, v2, a2 = [x[i:i + 100] for x in ops5]
            head(prime, v1, a1, images_v2=v2, audios_v2=None, normalized=False)
    assert head.report() == str(g["report"])


@pytest.mark.parametrize("B", [130, 800])
def test_head_under_a_frozen_image_tower(B):
    """`model.image.freeze=True` (the config default): the image views carry no gradient, so vp and vv produce none and only the
    audio view's is asked for -- on the fused path and, at B = 800, through the single-pair launches."""
    from vipant_amd import module as M
    head = M.build_loss_head(loss_cfg()).to(DEV).train()
    prime, v1, a1, v2 = features(B, 4, B)
    a1.requires_grad_()
    loss = head(prime, v1, a1, images_v2=v2, normalized=False)
    loss.backward()
    assert all(getattr(head, f"loss_head_{k}").logit_scale.grad is not None for k in ("vp", "va", "vv"))
    x64 = a1.detach().double().requires_grad_()
    xn = [t.double() / t.double().norm(dim=-1, keepdim=True) for t in (prime, v1)] + [x64 / x64.norm(dim=-1, keepdim=True)] \
        + [v2.double() / v2.double().norm(dim=-1, keepdim=True)]
    ls = [float(getattr(head, f"loss_head_{k}").logit_scale) for k in ("vp", "va", "vv")]
    losses, total, dxn, emun, _ = reference([x.detach().float() for x in xn], [(1, 0), (1, 2), (1, 3)], ls, [0.0] * 3, [1.0] * 3, 1.0)
    assert abs(float(loss.detach()) - total) <= 1e-3
    ref, = torch.autograd.grad(xn[2], x64, dxn[2], retain_graph=True)
    emu, = torch.autograd.grad(xn[2], x64, emun[2])
    (hl2, hmx), (el2, emx) = errs(a1.grad, ref), errs(emu, ref)
    print(f"[vace frozen image B={B}] da1: rel L2 hip={hl2:.3e} emu={el2:.3e}; max-abs hip={hmx:.3e} emu={emx:.3e}")
    assert hl2 <= 1.5 * el2 + 1e-3 and hmx <= 1.5 * emx + 1e-3


def test_none_rules_eval_routing_and_report_prefixes():
    from vipant_amd import module as M
    head = M.build_loss_head(loss_cfg(ap=True)).to(DEV).train()
    prime, v1, a1, v2 = features(40, 4, 7)
    loss = head(None, v1.requires_grad_(), a1, images_v2=None)           # only va is live: no prime features, no second view
    assert float(head._total_loss["va"]) == float(loss) and float(head._total_loss["vp"]) == 0.0 == float(head._total_loss["vv"])
    head.copy_state_dict({"loss_head_va.logit_scale": torch.zeros(())})   # a no-op, as in the reference
    assert float(head.loss_head_va.logit_scale) != 0.0
    head.eval()
    with torch.no_grad():
        assert head(prime, v1, a1, images_v2=v2, audios_v2=None, normalized=False) == 0.
    rep = head.report()
    tags = re.findall(r"^(VP|AP|VA|VV|AA): I->A: t1 = \d+\.\d\d t5 = \d+\.\d\d A->I: t1 = \d+\.\d\d t5 = \d+\.\d\d @ 40$", rep, flags=re.M)
    assert rep.startswith("\nVP: ") and tags == ["VP", "AP", "VA", "VV"], rep


def _monitor(extra=""):
    from vipant_amd.config import compose
    from vipant_amd.monitor import VASMonitor
    cfg = compose((OV + " " + extra).split())
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    lines = []
    return VASMonitor(cfg, lambda m: lines.append(str(m)), torch.device(DEV)), lines


def test_both_image_views_as_one_batch_equal_two_passes_and_four_steps_train():
    mon, lines = _monitor()
    model = mon.model
    assert type(model).__name__ == "CVASP" and any(p.requires_grad for p in model.image_head.parameters())
    batch = mon.make_batch(next(iter(mon.dataloader)))
    images, v1, v2, a1, a2, _ = batch
    assert a2 is None and images.shape == (4, 512) and v1.shape == v2.shape == (4, 3, 224, 224) and a1.shape == (4, 1, 256, 64)
    with torch.no_grad():
        f1, f2 = model.encode_views(v1, v2, normalized=True)
        g1, g2 = model.image_head(v1, normalized=True), model.image_head(v2, normalized=True)
    assert torch.equal(f1, g1) and torch.equal(f2, g2)
    before = {k: p.detach().clone() for k, p in model.named_parameters() if p.requires_grad}
    mon.learn()
    torch.cuda.synchronize()
    text = "\n".join(lines)
    steps = re.findall(r"step (\d)\tlr_w \S+ lr_b \S+ loss (\d+\.\d{3}) vp (\d+\.\d{3}) va (\d+\.\d{3}) vv (\d+\.\d{3}) \d+\.\d\d samples/s", text)
    print(text)
    assert [int(s[0]) for s in steps] == [1, 2, 3, 4], text
    vals = torch.tensor([[float(x) for x in s[1:]] for s in steps])
    assert torch.isfinite(vals).all()
    assert torch.allclose(vals[:, 0], vals[:, 1:].sum(1), atol=2e-3)            # weights 1: the total is the sum of the three terms
    assert "# step 4 # sample 16" in text and mon.total_inst == 16
    moved = [k for k, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[k])]
    assert any(k.startswith("image_head.") for k in moved) and any(k.startswith("audio_head.") for k in moved)
    assert sum(k.startswith("loss_head.") for k in moved) == 3


def test_shared_encoder_gradients_are_the_sum_over_both_towers():
    """running.siamese.alive=True amodules=[encoder]: the audio tower runs the IMAGE tower's blocks.  One step's gradient of every
    shared block parameter equals the sum of the gradient through the image tower alone and through the audio tower alone (the
    other tower's features detached) -- up to the fp32 rounding of that one addition, relative to the parameter's largest
    gradient entry: 2 x 2^-24 per term, 1e-6 asked."""
    mon, _ = _monitor("running.siamese.alive=True running.siamese.amodules=[encoder]")
    model = mon.model
    assert model.audio_head.encoder is model.image_head.encoder
    images, v1, v2, a1, _, _ = mon.make_batch(next(iter(mon.dataloader)))
    shared = dict(model.image_head.encoder.named_parameters())

    def grads(image_path, audio_path):
        for p in model.parameters():
            p.grad = None
        kw = {"normalized": True}
        f1, f2 = model.encode_views(v1, v2, **kw)
        fa = model.audio_head(a1, **kw)
        if not image_path:
            f1, f2 = f1.detach(), f2.detach()
        if not audio_path:
            fa = fa.detach()
        prime = images / images.norm(dim=-1, keepdim=True)
        model.loss_head(prime, f1, fa, images_v2=f2, audios_v2=f2, **kw).backward()
        return {k: p.grad.detach().clone() for k, p in shared.items()}
    both, img, aud = grads(True, True), grads(True, False), grads(False, True)
    for k in shared:
        scale = float(both[k].abs().max())
        assert scale > 0 and float(img[k].abs().max()) > 0 and float(aud[k].abs().max()) > 0, k
        err = float((both[k] - (img[k] + aud[k])).abs().max())
        assert err <= 1e-6 * scale, (k, err, scale)
    mon.step(images, v1, v2, a1, None)            # and a whole step runs: every shared parameter moves
    torch.cuda.synchronize()


def test_four_steps_through_the_train_entry(tmp_path):
    """train.py with the issue's override line (shrunk towers, synthetic five-slot batches): four steps, a finite loss, a
    well-formed `stats` part in every log line and the right sample count."""
    import math
    import train as entry
    entry.train((OV + f" alias_root={tmp_path} model_name=s mode=dp verbose=False running.peep_rate=1").split())
    torch.cuda.synchronize()
    text = (tmp_path / "s" / "train_0.out").read_text()
    steps = re.findall(r"step (\d)\tlr_w \S+ lr_b \S+ loss (\S+) vp (\d+\.\d{3}) va (\d+\.\d{3}) vv (\d+\.\d{3}) \d+\.\d\d samples/s", text)
    assert [int(s[0]) for s in steps] == [1, 2, 3, 4], text
    assert all(math.isfinite(float(s[1])) and re.fullmatch(r"\d+\.\d{3}", s[1]) for s in steps)
    assert "# step 4 # sample 16" in text


def test_e2e_cvasp_against_reference(golden):
    """CVASP.forward against the reference's glue run by hand (tests/golden/make_golden_siamese.py: the image tower once per view):
    loss and per-pair losses within 1e-3, the budget the 2-block end-to-end fixtures closest in size carry (`e2e_cls`,
    `e2e_barlow_ce`: tests/test_cls_golden_gpu.py, tests/test_barlow_golden_gpu.py) and the project's loss budget; features and tower gradients under the end-to-end rule of tests/test_cls_golden_gpu.py -- features 2 %
    of scale; on the five tensors that test checks, for BOTH towers, the norm within 5 % and rel-L2 of the sampled entries within
    0.15; d logit_scale of every pair rel 0.15."""
    import numpy as np
    import gen
    import gen_siamese as G
    from vipant_amd.config import compose
    from vipant_amd.model import CVASP
    fx = golden("e2e_siamese")
    tag, L, b, T_, Fq = "e2e_siamese", 2, 16, 256, 64
    cfg = compose((OV + f" running.batch_size={b}").split())
    model = CVASP(cfg, lambda *_: None)
    model.build()
    S = model.audio_head.misc.positional_embedding.shape[0]
    assert S == int(fx["S"])
    model.audio_head.load_state_dict({k: v.to(DEV) for k, v in gen.det_weights(f"{tag}/audio", gen.vit_head_shapes(768, L, 512, S)).items()}, strict=True)
    model.image_head.load_state_dict({k: v.to(DEV) for k, v in gen.det_weights(f"{tag}/image", gen.vit_head_shapes(768, L, 512, 50)).items()}, strict=True)
    model.train()
    prime = gen.det_randn(f"{tag}/prime", (b, 512))
    v1, v2 = G.e2e_views(tag, b)
    aud = gen.det_randn(f"{tag}/aud", (b, 1, T_, Fq))
    assert np.allclose(gen.checksum(aud), fx["aud_sum"]) and np.allclose(gen.checksum(v1), fx["v1_sum"])
    feats = {}
    model.image_head.register_forward_hook(lambda m, i, o: feats.__setitem__("i", o))
    model.audio_head.register_forward_hook(lambda m, i, o: feats.__setitem__("a", o))
    loss = model(prime.to(DEV), v1.to(DEV), aud.to(DEV), images_v2=v2.to(DEV))
    loss.backward()
    got = {"f1": feats["i"][:b], "f2": feats["i"][b:], "fa": feats["a"]}
    for k, f in got.items():
        want = torch.from_numpy(fx[k]).double()
        ferr = float((f.detach().double().cpu() - want).abs().max() / want.abs().max())
        print(f"[e2e_siamese] feature {k}: err {ferr:.2e} of scale")
        assert ferr < 2e-2, (k, ferr)
    lerr = abs(float(loss.detach()) - float(fx["loss"]))
    print(f"[e2e_siamese] loss hip={float(loss.detach()):.6f} reference={float(fx['loss']):.6f} diff {lerr:.2e}")
    for k in ("vp", "va", "vv"):
        d = abs(float(model.loss_head._total_loss[k]) - float(fx[f"loss_{k}"]))
        print(f"[e2e_siamese] {k}: diff {d:.2e}")
        assert d <= 1e-3, (k, d)
    assert lerr <= 1e-3, (float(loss.detach()), float(fx["loss"]))
    rel = lambda a, r: float(np.linalg.norm(np.asarray(a, dtype=np.float64).reshape(-1) - np.asarray(r, dtype=np.float64).reshape(-1))
                             / max(np.linalg.norm(np.asarray(r, dtype=np.float64)), 1e-30))
    for k, p in model.loss_head.named_parameters():
        e = rel(p.grad.detach().cpu().numpy(), fx[f"g_{k}"])
        print(f"[e2e_siamese] head gradient {k}: rel {e:.2e}")
        assert e < 0.15, (k, e)
    checked = ("misc.class_embedding", "misc.positional_embedding", "post_encoder.proj", "pre_encoder.conv1.weight",
               "encoder.resblocks.0.attn.in_proj_bias")
    for pre, head in (("a_", model.audio_head), ("i_", model.image_head)):
        out = {}
        for k, p in head.named_parameters():
            g = p.grad.detach().double().cpu().reshape(-1)
            idx = torch.from_numpy(fx[f"{pre}idx_{k}"])
            e = rel(g[idx].numpy(), fx[f"{pre}s_{k}"])
            n = (float((g * g).sum()) / float(fx[f"{pre}sum_{k}"][1])) ** 0.5
            out[k] = (e, n)
            if k in checked:
                assert abs(n - 1) < 5e-2 and e < 0.15, (pre, k, e, n)
        print(f"[e2e_siamese] {pre} tower gradients (rel-L2 of the sampled entries, norm ratio): "
              + ", ".join(f"{k}=({e:.2e}, {n:.3f})" for k, (e, n) in out.items() if k in checked))
