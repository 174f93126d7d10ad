"""Transformer towers at widths that are no multiple of 256 (ViT-Ti 192, ViT-S 384, the RN50x4 text tower's 640) against the CPU
restatement (oracle/ref_cpu.py): the stack with the bounds of tests/test_model_gpu.py::test_backbone_other_widths_match_oracle, one
whole audio head of width 384 with those of test_pre_post_golden; the widths and the e4m3 request a tower refuses when it is built."""
from types import SimpleNamespace as NS

import pytest
import torch

import gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def M():
    import vipant_amd.module as mod
    from vipant_amd import _ffi
    _ffi.call("vipant_device_check")
    return mod


def rel_err(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("D,S,b,layers,causal", [(192, 17, 3, 1, False), (384, 50, 2, 2, False), (640, 77, 2, 1, True)])
def test_backbone_matches_oracle(M, D, S, b, layers, causal):
    from oracle import ref_cpu as R
    ctx = 77 if causal else None
    bb = M.TransformerBackbone(NS(layers=layers, skip_attn_mask=not causal), width=D, ctx_len=ctx)
    sd = {k[len("encoder."):]: v for k, v in gen.det_weights(f"widths/{D}", gen.backbone_shapes(D, layers)).items()}
    bb.load_state_dict(sd, strict=True)
    bb = bb.to(DEV)
    x, gy = gen.det_randn(f"widths/{D}/x", (b, S, D)), gen.det_randn(f"widths/{D}/gy", (b, S, D))
    xr = x.clone().requires_grad_()
    sdr = {k: v.clone().requires_grad_() for k, v in sd.items()}
    yr = R.transformer_backbone(xr, sdr, "", layers, D, ctx, not causal)
    yr.backward(gy)
    xg = x.to(DEV).requires_grad_()
    y = bb(xg)
    y.backward(gy.to(DEV))
    assert rel_err(y, yr.detach()) < 2e-2, rel_err(y, yr.detach())
    assert rel_err(xg.grad, xr.grad) < 4e-2, rel_err(xg.grad, xr.grad)
    for k, p in bb.named_parameters():
        assert rel_err(p.grad, sdr[k].grad) < 5e-2, (k, rel_err(p.grad, sdr[k].grad))


def audio_cfg(width, layers, **kw):
    return NS(name="CLIPAudioHead", width=width, embed_dim=512, resolution=[64, 64], ctx_len=77,
              encoder=NS(name="TransformerBackbone", layers=layers, skip_attn_mask=True),
              pre_encoder=NS(name="ViTPreEncoder", patch_size=16, stride=[16, 16], in_channels=3),
              post_encoder=NS(name="ViTPostEncoder"), misc=NS(name="CLIPMisc"),
              pre_encoder_addon=NS(name="AddonEncoder"), post_encoder_addon=NS(name="AddonEncoder"), **kw)


def test_audio_head_384_matches_oracle(M):
    """Patch embedding + ln_pre (vipant_patch_embed_ln_*), two blocks, read-out (vipant_cls_ln_proj_l2norm_*), forward and backward."""
    from oracle import ref_cpu as R
    D, b = 384, 3
    head = M.build_audio_head(audio_cfg(D, 2))
    S = head.misc.positional_embedding.shape[0]
    sd = gen.det_weights("widths/head384", gen.vit_head_shapes(D, 2, 512, S, patch=16))
    head.load_state_dict(sd, strict=True)
    head = head.to(DEV)
    sdr = {k: v.clone().requires_grad_() for k, v in sd.items()}
    x = gen.det_randn("widths/head384/x", (b, 1, 64, 64))
    pre = head.pre_encoder(x.to(DEV), positional_embedding=head.misc.pos_embedding, class_embedding=head.misc.cls_embedding)
    pre_r = R.vit_pre_encoder(x, sdr, [16, 16], sdr["misc.positional_embedding"], sdr["misc.class_embedding"])
    assert rel_err(pre, pre_r.detach()) < 1e-2, rel_err(pre, pre_r.detach())
    gp = gen.det_randn("widths/head384/gpre", tuple(pre.shape))
    pre.backward(gp.to(DEV))
    pre_r.backward(gp)
    grads = {"misc.positional_embedding": (head.misc.positional_embedding, 1e-3), "misc.class_embedding": (head.misc.class_embedding, 1e-3),
             "pre_encoder.ln.weight": (head.pre_encoder.ln.weight, 1e-2), "pre_encoder.ln.bias": (head.pre_encoder.ln.bias, 1e-3),
             "pre_encoder.conv1.weight": (head.pre_encoder.conv1.weight, 2e-2)}
    for k, (p, bound) in grads.items():
        assert rel_err(p.grad, sdr[k].grad) < bound, (k, rel_err(p.grad, sdr[k].grad))
    h = gen.det_randn("widths/head384/h", (b, S, D))
    hg = h.to(DEV).requires_grad_()
    post = head.post_encoder(hg)
    post_r = R.vit_post_encoder(h, sdr)
    assert rel_err(post, post_r.detach()) < 1e-2, rel_err(post, post_r.detach())
    go = gen.det_randn("widths/head384/gpost", tuple(post.shape))
    post.backward(go.to(DEV))
    post_r.backward(go)
    assert rel_err(head.post_encoder.ln.weight.grad, sdr["post_encoder.ln.weight"].grad) < 1e-2
    with torch.no_grad():       # the whole head: test_image_head_golden's bound on the normalised feature
        feat = head(x.to(DEV), normalized=True)
        feat_r = R.vit_head_forward(x, sd, width=D, layers=2, stride=[16, 16], position_resolution=head.misc.position_resolution)
    assert rel_err(feat, feat_r) < 2e-2, rel_err(feat, feat_r)


def test_widths_refused_when_the_tower_is_built(M):
    from vipant_amd.errors import VipantError
    for width in (128, 200):
        with pytest.raises(VipantError, match="multiple of 64 from 192 to 1024"):
            M.TransformerBackbone(NS(layers=1, skip_attn_mask=True), width=width, ctx_len=None)
        with pytest.raises(VipantError, match="multiple of 64 from 192 to 1024"):
            M.build_audio_head(audio_cfg(width, 1))
    bb = M.TransformerBackbone(NS(layers=1, skip_attn_mask=True), width=384, ctx_len=None)
    with pytest.raises(VipantError, match="256, 512, 768 and 1024"):
        bb.fp8 = True           # what running.fp8_gemm=True sets on the audio tower (Monitor._configure)
    M.TransformerBackbone(NS(layers=1, skip_attn_mask=True), width=512, ctx_len=None).fp8 = True
