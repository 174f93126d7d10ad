"""Patchout through the public interface: a 2-block width-192 CLIPAudioHead from config with `+model.audio.pre_encoder.patchout.keep=0.5`
against a float64 restatement on the kept tokens: relative L2 error within 1.5 x that of its bf16-operand emulation + 1e-3."""
import pytest
import torch
import torch.nn.functional as Fn

from test_barlow_gpu import _RoundBwd, _RoundFwd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T, F, PATCH, LAYERS = 3, 64, 48, 16, 2


def build(width=192, patchout="+model.audio.pre_encoder.patchout.keep=0.5"):
    import vipant_amd.module as M
    from vipant_amd.config import compose
    cfg = compose(f"+running=bimodal +running/audio=default +model/image=vit_val +model/audio=vit_val +model/text=dummy model.image.width={width} "
                  f"model.image.encoder.layers={LAYERS} model.image.pre_encoder.patch_size={PATCH} model.audio.resolution=[{T},{F}] "
                  f"{patchout}".split())
    torch.manual_seed(width)
    head = M.build_audio_head(cfg.model.audio)
    head.encoder.stream_f16 = False         # running.stream_dtype=fp32: the restatement below has no fp16 stream
    return head


def restate(sd, x, keep, gy, emulate):
    """float64: patch conv on the kept patches (channel-mean kernel), cls, pos, ln_pre, the blocks, ln_post(cls row) @ proj; emulate: every
    contraction operand rounded to bf16, forward and backward.  -> (feature, {name: gradient})."""
    rf, rg = (_RoundFwd.apply, _RoundBwd.apply) if emulate else ((lambda t: t),) * 2
    p = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    ln = lambda t, n: Fn.layer_norm(t, t.shape[-1:], p[n + ".weight"], p[n + ".bias"], 1e-5)
    mm = lambda a, n: rg(a @ rf(p[n]).t())
    D = p["misc.class_embedding"].shape[0]
    pos, idx = p["misc.positional_embedding"], keep.long()
    cols = Fn.unfold(rf(x.double()), PATCH, stride=PATCH).transpose(1, 2)
    A = torch.gather(cols, 1, idx.unsqueeze(2).expand(-1, -1, cols.shape[2]))
    tok = rg(A @ rf(p["pre_encoder.conv1.weight"].mean(1).reshape(D, -1)).t()) + pos[1 + idx]
    h = ln(torch.cat([(p["misc.class_embedding"] + pos[0]).expand(B, 1, D), tok], 1), "pre_encoder.ln")
    S, H = h.shape[1], D // 64
    for l in range(LAYERS):
        h = rg(h)       # the residual stream's gradient crosses every block boundary as bf16 (running.grad_stream, default bf16)
        n = f"encoder.resblocks.{l}."
        qkv = rf(mm(rf(ln(h, n + "ln_1")), n + "attn.in_proj_weight") + p[n + "attn.in_proj_bias"])
        q, k, v = (t.reshape(B, S, H, 64).transpose(1, 2) for t in qkv.chunk(3, -1))
        o = rf((torch.softmax(rg(q @ k.transpose(-1, -2)) / 8.0, -1) @ v).transpose(1, 2).reshape(B, S, D))
        h = h + rf(mm(o, n + "attn.out_proj.weight") + p[n + "attn.out_proj.bias"])
        u = mm(rf(ln(h, n + "ln_2")), n + "mlp.c_fc.weight") + p[n + "mlp.c_fc.bias"]
        h = h + rf(mm(rf(u * torch.sigmoid(1.702 * u)), n + "mlp.c_proj.weight") + p[n + "mlp.c_proj.bias"])
    feat = rg(rf(ln(h[:, 0], "post_encoder.ln")) @ rf(p["post_encoder.proj"]))
    feat.backward(gy.double())
    return feat.detach(), {k: v.grad for k, v in p.items()}


def rel(a, b):
    return float((a.detach().double().cpu() - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("kind", ["drawn", "shared"])
def test_train_step_matches_fp64_on_the_kept_tokens(kind):
    from vipant_amd import ops
    head = build()
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    head = head.to(DEV).train()
    g = torch.Generator().manual_seed(5)
    x, gy = torch.randn(B, 1, T, F, generator=g), torch.randn(B, 512, generator=g)
    keep = ops.draw_patchout(B if kind == "drawn" else 1, T // PATCH, F // PATCH, keep=0.5, generator=g).expand(B, -1).contiguous()
    feat = head(x.to(DEV), keep=keep)
    feat.backward(gy.to(DEV))
    ref, emu = restate(sd, x, keep, gy, False), restate(sd, x, keep, gy, True)
    got = dict({k: p.grad for k, p in head.named_parameters()}, feature=feat)
    for k, v in got.items():
        e_hip, e_emu = (rel(v, ref[0]), rel(emu[0], ref[0])) if k == "feature" else (rel(v, ref[1][k]), rel(emu[1][k], ref[1][k]))
        print(f"[patchout {kind}] {k}: kernels {e_hip:.3e}, emulation {e_emu:.3e}")
        assert e_hip <= 1.5 * e_emu + 1e-3, (k, e_hip, e_emu)


def test_eval_and_no_grad_see_every_patch():
    head, plain = build(), build(patchout="")
    plain.load_state_dict(head.state_dict(), strict=True)
    head, plain = head.to(DEV), plain.to(DEV)
    x = torch.randn(B, 1, T, F, generator=torch.Generator().manual_seed(6)).to(DEV)
    assert torch.equal(head.eval()(x), plain.eval()(x))
    with torch.no_grad():
        assert torch.equal(head.train()(x), plain.train()(x))


def test_structured_draw_and_refusals():
    from vipant_amd import ops
    from vipant_amd.errors import VipantError
    nrow, ncol = 7, 5
    keep = ops.draw_patchout(4, nrow, ncol, time=2, freq=1, generator=torch.Generator().manual_seed(3))
    assert keep.dtype == torch.int32 and tuple(keep.shape) == (4, (nrow - 2) * (ncol - 1))
    for row in keep.tolist():
        rows, cols = sorted({p // ncol for p in row}), sorted({p % ncol for p in row})
        assert len(rows) == nrow - 2 and len(cols) == ncol - 1 and row == [r * ncol + c for r in rows for c in cols]
    for bad in (dict(keep=0), dict(keep=36), dict(time=7), dict(keep=3, time=1)):
        with pytest.raises(VipantError):
            ops.draw_patchout(2, nrow, ncol, **bad)
    with pytest.raises(VipantError, match="patchout"):
        build(width=256).encoder.fp8 = True         # what running.fp8_gemm=True sets on the audio tower
