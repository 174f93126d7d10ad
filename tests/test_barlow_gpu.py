"""Barlow Twins loss heads on the MI355X (model/loss=barlow, barlow_ce; cvap/module/decoder/loss_head.py:287-328, 601-622).

Kernel level: batch norm forward / backward and the cross-correlation loss against fp64 on fp32 inputs (fp32 rounding only:
statistics, column sums and loss parts to 1e-5; bf16 outputs to one bf16 rounding).  Head level: against a float64 restatement of
the reference head, with the gradient budget computed by the test itself -- 1.5 x the error of the same restatement with the
HIP path's bf16 operands (forward values and backward operands rounded where the kernels round them) + 1e-3.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from vipant_amd import _ffi, ops as O
    _ffi.call("vipant_device_check")
    return O


def rnd(*shape, scale=1.0, shift=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale + shift


def bf16_close(got, ref, what, atol):
    """bf16 output against fp64: one bf16 rounding (2^-8 relative) + atol."""
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    bad = err > 2.0 ** -8 * ref.abs() + atol
    assert not bad.any(), (what, int(bad.sum()), float(err.max()))


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------ batch norm kernels
def bn_ref(x, g, b, relu):
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    y = (x - mean) * rstd
    if g is not None:
        y = y * g + b
    return (y.clamp_min(0) if relu else y), mean, rstd


CASES = [(M, N) for M in (2, 3, 64, 257, 4096) for N in (64, 192, 4096)]


@pytest.mark.parametrize("M,N", CASES)
def test_batchnorm_fwd_bwd_against_fp64(ops, M, N):
    seed = M * 7 + N
    x = rnd(M, N, scale=1.5, shift=3.0, seed=seed)            # column means far from 0: the shifted statistics must hold
    for variant, (affine, relu) in enumerate(((False, False), (True, False), (True, True))):
        g = rnd(N, scale=0.5, shift=1.0, seed=seed + 1) if affine else None
        b = rnd(N, scale=0.5, seed=seed + 2) if affine else None
        dy = rnd(M, N, seed=seed + 3 + variant)
        rm, rv = rnd(N, seed=seed + 4), rnd(N, seed=seed + 5).abs() + 0.5
        nbt = torch.zeros((), dtype=torch.int64)
        xd = x.to(DEV)
        gd, bd = (g.to(DEV), b.to(DEV)) if affine else (None, None)
        rmd, rvd, nbtd = rm.to(DEV), rv.to(DEV), nbt.to(DEV)
        y, mean, rstd = ops.batchnorm_fwd(xd, gd, bd, relu=relu, running_mean=rmd, running_var=rvd, num_batches_tracked=nbtd)
        x2 = (x * 0.5 - 1.0)
        ops.batchnorm_fwd(x2.to(DEV), gd, bd, relu=relu, running_mean=rmd, running_var=rvd, num_batches_tracked=nbtd)
        # fp64 reference
        yr, mr, rr = bn_ref(x.double(), g.double() if affine else None, b.double() if affine else None, relu)
        gam = g.double() if affine else torch.ones(N, dtype=F64)
        # fp32 rounding of the inputs: x - mean carries up to ~ulp(|x|), i.e. xhat up to 4 ulp(max |x|) * rstd per column
        # (large when a column's rows nearly agree, M = 2), and gamma * xhat + beta may cancel below that
        xerr = 4 * 2.0 ** -24 * x.abs().max(0).values.double() * rr
        bf16_close(y, yr, f"y {variant}", atol=1e-6 + xerr * gam.abs())
        assert rel(mean, mr) <= 1e-5 and rel(rstd, rr) <= 1e-5, variant
        # two running-statistics updates (momentum 0.1, unbiased variance)
        ref_m, ref_v = rm.double(), rv.double()
        for xi in (x.double(), x2.double()):
            ref_m = 0.9 * ref_m + 0.1 * xi.mean(0)
            ref_v = 0.9 * ref_v + 0.1 * xi.var(0, unbiased=True)
        assert rel(rmd, ref_m) <= 1e-5 and rel(rvd, ref_v) <= 1e-5, variant
        assert int(nbtd) == 2
        # backward, in fp64 with the ReLU mask of the kernel's own forward (an element within fp32 rounding of the kink may
        # go either way, and then carries its whole gradient); affine: a row range for the parameter sums
        r0, nr = (M // 3, max(1, M // 2)) if affine else (0, M)
        dg = torch.zeros(N, device=DEV) if affine else None
        db = torch.zeros(N, device=DEV) if affine else None
        dx = ops.batchnorm_bwd(dy.to(DEV), xd, mean, rstd, gd, bd, relu=relu, dgamma=dg, dbeta=db, row0=r0, nrows=nr)
        xhat = (x.double() - mr) * rr
        gm = dy.double() * (y.cpu() > 0) if relu else dy.double()
        dx_ref = rr * gam * (gm - gm.mean(0) - xhat * (gm * xhat).mean(0))
        bf16_close(dx, dx_ref, f"dx {variant}", atol=(rr * gam).abs() * (1e-5 + xerr) * float(dy.abs().max()))
        if affine:
            assert rel(dg, (gm * xhat)[r0:r0 + nr].sum(0)) <= 1e-5
            assert rel(db, gm[r0:r0 + nr].sum(0)) <= 1e-5


def test_batchnorm_is_bit_identical_run_to_run_and_refuses_one_row(ops):
    from vipant_amd._ffi import VipantError
    x = rnd(4096, 4096, scale=2.0, shift=1.0, seed=11).to(DEV)
    g, b = rnd(4096, seed=12).to(DEV), rnd(4096, seed=13).to(DEV)
    dy = rnd(4096, 4096, seed=14).to(DEV)
    outs = []
    for _ in range(2):
        y, mean, rstd = ops.batchnorm_fwd(x, g, b, relu=True)
        dg, db = torch.empty(4096, device=DEV), torch.empty(4096, device=DEV)
        dx = ops.batchnorm_bwd(dy, x, mean, rstd, g, b, relu=True, dgamma=dg, dbeta=db)
        outs.append([t.clone() for t in (y, mean, rstd, dx, dg, db)])
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    with pytest.raises(VipantError, match="M >= 2"):
        ops.batchnorm_fwd(x[:1], g, b)


# ------------------------------------------------------------------------------------------------ loss kernel
@pytest.mark.parametrize("N", [64, 192, 4096])
def test_barlow_loss_kernel_against_fp64(ops, N):
    M, lambd = 37, 0.0051
    c = rnd(N, N, scale=4.0, seed=N) + torch.eye(N) * M * 0.8
    scale = torch.tensor([0.37])
    out, G, Gt = ops.barlow_loss(c.to(DEV), M, lambd, grad_scale=scale.to(DEV), want_grad=True)
    cd = c.double() / M
    eye = torch.eye(N, dtype=torch.bool)
    on = ((cd.diagonal() - 1) ** 2).sum()
    off = cd[~eye].pow(2).sum()
    out = out.cpu().double()
    assert abs(float(out[1] - on)) <= 1e-5 * float(on) and abs(float(out[2] - off)) <= 1e-5 * float(off)
    assert abs(float(out[0] - (on + lambd * off))) <= 1e-5 * float(on + lambd * off)
    gref = torch.where(eye, 2 * (cd - 1), 2 * lambd * cd) * 0.37 / M
    bf16_close(G, gref, "G", atol=1e-6 * 0.37 / M)
    assert torch.equal(Gt.cpu(), G.cpu().t())
    again, G2, _ = ops.barlow_loss(c.to(DEV), M, lambd, grad_scale=scale.to(DEV), want_grad=True)
    assert torch.equal(again.cpu().double(), out) and torch.equal(G2, G)


# ------------------------------------------------------------------------------------------------ heads
class _RoundFwd(torch.autograd.Function):          # a bf16 operand: the value is rounded, its gradient is not
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):          # a gradient the HIP path hands to a contraction as a bf16 operand
    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def _bn(y, g, b, rm, rv):
    mean, var = y.mean(0), y.var(0, unbiased=False)
    with torch.no_grad():
        rm.mul_(0.9).add_(0.1 * mean)
        rv.mul_(0.9).add_(0.1 * y.var(0, unbiased=True))
    out = (y - mean) / torch.sqrt(var + 1e-5)
    return out * g + b if g is not None else out


def ref_barlow(sd, L, x1, x2, lambd, emulate):
    """float64 restatement of BarlowLossHead.forward in training mode (loss_head.py:313-328, one process): returns
    (loss, on, off, params {name: leaf}, running {name: buffer}, x1, x2 leaves)."""
    rf = _RoundFwd.apply if emulate else (lambda t: t)
    rg = _RoundBwd.apply if emulate else (lambda t: t)
    P = {k: v.double().clone().requires_grad_() for k, v in sd.items() if not k.endswith(("running_mean", "running_var",
                                                                                          "num_batches_tracked"))}
    R = {k: v.double().clone() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))}
    x1, x2 = x1.double().requires_grad_(), x2.double().requires_grad_()
    W = [rf(P[f"linear.{3 * i}.weight"]) for i in range(L + 1)]

    def proj(x):
        h = rf(x)
        for i in range(L):
            n = f"linear.{3 * i + 1}"
            y = rg(h @ W[i].t())
            h = rf(torch.relu(_bn(y, P[n + ".weight"], P[n + ".bias"], R[n + ".running_mean"], R[n + ".running_var"])))
        return rg(h @ W[L].t())

    z1, z2 = proj(x1), proj(x2)
    zn1 = rf(_bn(z1, None, None, R["bn.running_mean"], R["bn.running_var"]))
    zn2 = rf(_bn(z2, None, None, R["bn.running_mean"], R["bn.running_var"]))
    c = rg(zn1.t() @ zn2) / x1.shape[0]
    eye = torch.eye(c.shape[0], dtype=torch.bool)
    on = (c.diagonal() - 1).pow(2).sum()
    off = c[~eye].pow(2).sum()
    return on + lambd * off, on, off, P, R, x1, x2


def _barlow_cfg(layers, E=512):
    from vipant_amd.config import to_config
    return to_config({"name": "BarlowLossHead", "embed_dim": E, "lambd_off": 0.0051, "layers": list(layers)})


def _make_head(layers, seed):
    import vipant_amd.module as M
    torch.manual_seed(seed)
    head = M.build_loss_head(_barlow_cfg(layers))
    with torch.no_grad():                   # non-trivial affine parameters
        for m in head.linear:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(1.0 + 0.2 * torch.randn_like(m.weight))
                m.bias.copy_(0.1 * torch.randn_like(m.bias))
    return head


def _inputs(B, seed, E=512):
    x1 = rnd(B, E, seed=seed)
    return x1, x1 + 0.5 * rnd(B, E, seed=seed + 1)


def _check_head(B, layers, seed, want_x1_grad=True):
    head = _make_head(layers, seed)
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    L = len(layers) - 1
    x1, x2 = _inputs(B, seed)
    head = head.to(DEV).train()
    x1d = x1.to(DEV).requires_grad_(want_x1_grad)
    x2d = x2.to(DEV).requires_grad_()
    loss = head(x1d, x2d, normalized=False)
    loss.backward()
    ref = ref_barlow(sd, L, x1, x2, 0.0051, emulate=False)
    emu = ref_barlow(sd, L, x1, x2, 0.0051, emulate=True)
    for r in (ref, emu):
        r[0].backward()
    parts = head.parts.cpu().double()
    assert abs(float(loss) - float(ref[0])) <= 1e-3 * abs(float(ref[0])), (float(loss), float(ref[0]))
    for i in (1, 2):      # the two parts: each within the bf16-emulation's own distance (+ 1e-3), they may cancel in the sum
        e_hip, e_emu = abs(float(parts[i]) - float(ref[i])), abs(float(emu[i]) - float(ref[i]))
        assert e_hip <= 1.5 * e_emu + 1e-3 * float(ref[i]), (i, e_hip, e_emu)
    params = dict(head.named_parameters())
    report = {}
    for k, p in ref[3].items():
        e_hip, e_emu = rel(params[k].grad, p.grad), rel(emu[3][k].grad, p.grad)
        report[k] = (e_hip, e_emu)
        assert e_hip <= 1.5 * e_emu + 1e-3, (k, e_hip, e_emu)
    grads = ((x1d.grad, ref[5].grad, emu[5].grad, "dx1"), (x2d.grad, ref[6].grad, emu[6].grad, "dx2"))
    for got, r64, re, name in grads[(0 if want_x1_grad else 1):]:
        e_hip, e_emu = rel(got, r64), rel(re, r64)
        report[name] = (e_hip, e_emu)
        assert e_hip <= 1.5 * e_emu + 1e-3, (name, e_hip, e_emu)
    if not want_x1_grad:
        assert x1d.grad is None
    bufs = dict(head.named_buffers())
    for k, v in emu[4].items():
        report[k] = rel(bufs[k], v)
        assert rel(bufs[k], v) <= 1e-3, (k, rel(bufs[k], v))
        assert rel(bufs[k], ref[4][k]) <= 2e-2, k
    assert all(int(v) == 2 for k, v in bufs.items() if k.endswith("num_batches_tracked"))
    print(f"[barlow B={B} layers={layers}] loss hip={float(loss):.6f} fp64={float(ref[0]):.6f}; rel err (hip, bf16-emulation): "
          + ", ".join(f"{k}={v}" for k, v in report.items()))
    return head


def test_barlow_head_small_against_fp64():
    _check_head(48, [256, 512, 512], seed=5)


def test_barlow_head_reference_layers_against_fp64():
    _check_head(256, [2048, 4096, 4096], seed=6)


def test_barlow_head_frozen_image_features_skip_dx1():
    _check_head(64, [256, 512, 512], seed=7, want_x1_grad=False)


def test_barlow_head_is_bit_identical_run_to_run():
    outs = []
    for _ in range(2):
        head = _make_head([256, 512, 512], seed=8).to(DEV).train()
        x1, x2 = _inputs(64, 9)
        x2 = x2.to(DEV).requires_grad_()
        loss = head(x1.to(DEV), x2, normalized=False)
        loss.backward()
        outs.append([loss.detach().clone(), x2.grad.clone()] + [p.grad.clone() for p in head.parameters()]
                    + [b.clone() for b in head.buffers()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_barlow_ce_head_against_fp64(caplog):
    import logging
    import vipant_amd.module as M
    from vipant_amd.config import to_config
    cfg = to_config({"name": "BarlowCELossHead", "lambd_barlow": 0.05, "ce": {"name": "CELossHead"},
                     "barlow": dict(_barlow_cfg([256, 512, 512]))})
    torch.manual_seed(3)
    with caplog.at_level(logging.WARNING):
        head = M.build_loss_head(cfg)
    assert "scaling" in caplog.text
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    B = 64
    x1, x2 = _inputs(B, 21)
    head = head.to(DEV).train()
    x2d = x2.to(DEV).requires_grad_()
    loss = head(x1.to(DEV), x2d, normalized=False)
    loss.backward()
    bsd = {k[len("loss_barlow."):]: v for k, v in sd.items() if k.startswith("loss_barlow.")}
    out = {}
    for emulate in (False, True):
        lb, _, _, P, _, r1, r2 = ref_barlow(bsd, 2, x1, x2, 0.0051, emulate)
        ls = sd["loss_ce.logit_scale"].double().clone().requires_grad_()
        a, b = F.normalize(r1, dim=-1), F.normalize(r2, dim=-1)
        logits = ls.exp() * a @ b.t()
        lab = torch.arange(B)
        lce = F.cross_entropy(logits, lab) + F.cross_entropy(logits.t(), lab)
        total = lce + 0.05 * lb
        total.backward()
        out[emulate] = (total, P, ls, r2)
    ref, emu = out[False], out[True]
    assert abs(float(loss) - float(ref[0])) <= 1e-3 * abs(float(ref[0]))
    params = dict(head.named_parameters())
    assert rel(params["loss_ce.logit_scale"].grad, ref[2].grad) <= 1.5 * rel(emu[2].grad, ref[2].grad) + 1e-3
    for k, p in ref[1].items():
        got = params["loss_barlow." + k].grad
        assert rel(got, p.grad) <= 1.5 * rel(emu[1][k].grad, p.grad) + 1e-3, k
    assert rel(x2d.grad, ref[3].grad) <= 1.5 * rel(emu[3].grad, ref[3].grad) + 1e-3


def test_eval_mode_reports_retrieval_like_the_ce_head():
    """Eval mode runs no projector: BarlowLossHead caches features (LossHead.infer), BarlowCELossHead delegates to its CE head;
    both reports equal the CE head's on the same features."""
    import vipant_amd.module as M
    from vipant_amd.config import to_config
    x1, x2 = _inputs(96, 31)
    ce = M.build_loss_head(to_config({"name": "CELossHead", "layers": [], "scaling": True, "scale_max": None})).to(DEV).eval()
    bar = _make_head([256, 512, 512], seed=1).to(DEV).eval()
    bce = M.build_loss_head(to_config({"name": "BarlowCELossHead", "lambd_barlow": 0.05, "ce": {"name": "CELossHead"},
                                       "barlow": dict(_barlow_cfg([256, 512, 512]))})).to(DEV).eval()
    before = {k: v.clone() for k, v in bar.state_dict().items()}
    with torch.no_grad():
        for h in (ce, bar, bce):
            for i in range(0, 96, 32):
                h(x1[i:i + 32].to(DEV), x2[i:i + 32].to(DEV), normalized=False)
    want = ce.report()
    assert want.endswith("@ 96") and bar.report() == want and bce.report() == want
    for k, v in bar.state_dict().items():
        assert torch.equal(v.cpu(), before[k].cpu()), k            # no running-statistics update in eval


# ------------------------------------------------------------------------------------------------ through the trainer
def _va_overrides(loss="barlow_ce", extra=()):
    return ("+running=bimodal worker=CVALP mode=dp eval=False num_gpus=1 +model/image=vit_val +model/audio=vit_val "
            f"+model/text=dummy +model/loss={loss} +optimizer=standard +running/audio=default "
            "model.audio.pre_encoder.stride=[16,24] model.image.encoder.layers=1 running.audio.max_len=256 "
            "running.audio.num_mel_bins=64 running.batch_size=16 running.epochs=2 running.frame_emb=synthetic "
            "running.synthetic_steps=3 running.save_epoch=False optimizer.warmup_epoch=1").split() + list(extra)


@pytest.mark.parametrize("loss", ["barlow_ce", "barlow"])
def test_monitor_steps_and_checkpoint_round_trip(tmp_path, loss):
    from vipant_amd.config import compose
    from vipant_amd.monitor import VAMonitor
    import vipant_amd.module as M
    cfg = compose(_va_overrides(loss, [f"alias_root={tmp_path}", "running.save_rate=3"]))
    cfg.rank = 0
    torch.manual_seed(cfg.seed)
    mon = VAMonitor(cfg, lambda *_: None, torch.device(DEV))
    lh = mon.model.loss_head
    bar = lh.loss_barlow if loss == "barlow_ce" else lh
    rm0 = bar.bn.running_var.clone()
    w0 = bar.linear[0].weight.detach().clone()
    ids = {id(p) for p in lh.parameters()}
    assert ids <= {id(p) for p in mon.params}                  # the projector trains
    losses = []
    import time
    mon.total_loss = mon.total_step = mon.total_inst = 0
    mon.start_time = time.time()
    from vipant_amd.module import adjust_learning_rate
    for step, batch in enumerate(mon.dataloader):
        images, audios, text, _, _ = mon.make_batch(batch)
        adjust_learning_rate(cfg.optimizer, mon.optimizer, mon.dataloader, step + 1)    # LARS starts at lr 0 (warm-up)
        losses.append(float(mon.step(images, audios, None)))
    assert len(losses) == 3 and all(math.isfinite(v) for v in losses), losses
    assert not torch.equal(rm0, bar.bn.running_var) and int(bar.bn.num_batches_tracked) == 6
    assert not torch.equal(w0, bar.linear[0].weight.detach())
    mon.save()
    ck = torch.load(os.path.join(str(tmp_path), cfg.model_name, f"{mon.total_step:08d}.pth"), weights_only=False)
    fresh = M.build_loss_head(cfg.model.loss)
    fresh.load_state_dict(ck["model"][-1], strict=True)
    for k, v in lh.state_dict().items():
        assert torch.equal(fresh.state_dict()[k], v.cpu()), k


def test_at_script_dummy_images_are_refused():
    """The Barlow heads need real image features: with dummy images (the AT script's layout) the first forward names the
    combination instead of failing on a shape."""
    from vipant_amd._ffi import VipantError
    import vipant_amd.module as M
    head = _make_head([256, 512, 512], seed=2).to(DEV).train()
    with pytest.raises(VipantError, match="VA-only"):
        head(None, torch.randn(8, 512, device=DEV), None, normalized=False)
    from vipant_amd.config import to_config
    bce = M.build_loss_head(to_config({"name": "BarlowCELossHead", "lambd_barlow": 0.05, "ce": {"name": "CELossHead"},
                                       "barlow": dict(_barlow_cfg([256, 512, 512]))})).to(DEV).train()
    with pytest.raises(VipantError, match="VA-only"):
        bce(None, torch.randn(8, 512, device=DEV), None, normalized=False)
