"""vipant_hinge_logits and BCHingeLossHead on the MI355X against nn.MultiLabelMarginLoss in float64 on sigmoid(s * z.double()), targets
as `convert_label` builds them (cvap/module/decoder/loss_more.py:150-166), gradients from float64 autograd.  Kernel bounds: loss, dscale
1e-5 relative + 1e-7; prob 2 ulp of fp32 at the reference value; dz the float64 value rounded to bf16, one bf16 unit allowed, plus
2^-53 s / B: float64 autograd forms 1 - p from the ROUNDED p (1.0 at x = +40), so the reference itself is off by up to 2^-54 s / B there.
Head: the rules of tests/test_cls_gpu.py; the cached scores against the sigmoid of the bf16-operand emulation's logits (the operands
the HIP contractions see: with unrounded operands the scaled logits alone differ by more than 2e-3)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import vipant_amd.module as M
from vipant_amd import _ffi, ops
from test_cls_gpu import _RoundBwd, _RoundFwd, rel
from vipant_amd.config import to_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LS = (0.0, float(np.float32(np.log(1 / 0.07))))
CASES = [(C, B, first) for C in (1, 63, 64, 65, 527) for B in (1, 5, 64) for first in (range(4) if B == 1 else (0,))]
CASES += [(C, 5, 0) for C in (200, 1000, 1100)]      # the other register depths (4, 16) and a row too wide for registers


def margin_loss(p, t, reduction="mean"):
    lab = torch.full(t.shape, -1, dtype=torch.long)      # convert_label
    for i in range(len(t)):
        lid = t[i].nonzero(as_tuple=True)[0]
        lab[i, :len(lid)] = lid
    return nn.MultiLabelMarginLoss(reduction=reduction)(p, lab)


def inputs(C, B, first, s):
    # scaled logits in [-8, 8], 30 % marks; rows 0, 1, 2 are of kind first + 0, 1, 2 -- 0: no positive, 1: all positive, 2: scaled
    # logits of +-40, 3 and up: ordinary.  -> z, uint8 marks, the same marks as fractions in fp32
    g = torch.Generator().manual_seed(1000 * C + 10 * B + first)
    z = (16 * torch.rand(B, C, generator=g) - 8) / s
    t = (torch.rand(B, C, generator=g) < 0.3).to(torch.uint8)
    for i in range(min(B, 3)):
        if i + first < 2:
            t[i] = i + first
        elif i + first == 2:
            z[i] = torch.where(torch.rand(C, generator=g) < 0.5, 40.0, -40.0) / s
    return z.float(), t, t * (0.1 + torch.rand(B, C, generator=g))


def run(z, t, ls, C, row0=0, nrows=None, grad=True, dirt=0, ldz=None, kind=None):
    """One call through the C ABI -> (rc, loss, dscale, dz [B, ld], prob [B, ld]) on the host.  Every output starts as NaN; z and prob
    have ld = C + 3 (z's pad is NaN), dz lies between two NaN guard rows, the workspace has exactly the queried size, filled with `dirt`."""
    B, ld, nan = z.shape[0], C + 3, float("nan")
    nrows = B - row0 if nrows is None else nrows
    zp, t = F.pad(z, (0, 3), value=nan).to(DEV), t.to(DEV)
    lsd = None if ls is None else torch.tensor([ls], device=DEV)
    loss, dls, prob = (torch.full(shape, nan, device=DEV) for shape in ((1,), (1,), (B, ld)))
    dz = torch.full((B + 2, ld), nan, dtype=torch.bfloat16, device=DEV)
    ws = torch.full((_ffi.query("vipant_hinge_logits_workspace_bytes", nrows),), dirt, dtype=torch.uint8, device=DEV)
    rc = _ffi.lib().vipant_hinge_logits(
        zp.data_ptr(), ld if ldz is None else ldz, t.data_ptr(), t.stride(0), int(t.is_floating_point()) if kind is None else kind,
        ops._ptr(lsd), loss.data_ptr(), dz[1:].data_ptr() if grad else None, ld, dls.data_ptr() if (grad and ls is not None) else None,
        prob.data_ptr(), ld, row0, nrows, 1.0, B, C, ws.data_ptr(), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert dz[0].isnan().all() and dz[-1].isnan().all()
    return rc, loss.cpu(), dls.cpu(), dz[1:-1].cpu(), prob.cpu()


def same(a, b, rows=slice(None)):      # tensor by tensor, bit for bit (a NaN equals a NaN)
    return all(torch.equal(u[rows].float().nan_to_num(nan=7.0), v[rows].float().nan_to_num(nan=7.0)) for u, v in zip(a, b))


def in_units(err, ref, bits):      # err over the spacing of a `bits`-bit significand at ref; nothing is allowed at ref = 0
    return torch.where(err <= 0, 0.0, err / (torch.ldexp(torch.ones_like(ref), torch.frexp(ref)[1] - bits) * (ref != 0)))


@pytest.mark.parametrize("ls", LS)
@pytest.mark.parametrize("C,B,first", CASES)
def test_kernel_against_fp64(C, B, first, ls):
    s = float(np.exp(ls))
    z, t8, tf = inputs(C, B, first, s)
    zd, lsd = z.double().requires_grad_(), torch.tensor(ls, dtype=torch.float64, requires_grad=True)
    rp = torch.sigmoid(lsd.exp() * zd)
    rl = margin_loss(rp, t8)
    rl.backward()
    rl = rl.detach()
    out = rc, loss, dls, dz, prob = run(z, t8, ls, C)
    rb = zd.grad.float().bfloat16().double()
    e_dz = in_units((dz[:, :C].double() - rb).abs() - 2.0 ** -53 * s / B, rb, 8)
    e_p = in_units((prob[:, :C].double() - rp.detach()).abs(), rp.detach(), 24)
    print(f"[hinge C={C} B={B} first={first} s={s:.4g}] loss {float(loss):.9g} fp64 {float(rl):.9g}; dscale {float(dls):.9g} "
          f"fp64 {float(lsd.grad):.9g}; dz {float(e_dz.max()):.3f} bf16 units; prob {float(e_p.max()):.3f} ulp")
    assert rc == 0 and abs(float(loss) - float(rl)) <= 1e-5 * abs(float(rl)) + 1e-7
    assert abs(float(dls) - float(lsd.grad)) <= 1e-5 * abs(float(lsd.grad)) + 1e-7 and float(e_dz.max()) <= 1.0 and float(e_p.max()) <= 2.0
    assert prob[:, C:].isnan().all() and not dz[:, C:].any()          # prob's pad is a guard, dz's pad columns are written as zeros
    # the same bits: fractional fp32 marks from another dirty workspace; forward only; NULL logit_scale at s = 1; a strip's rows
    assert same(run(z, tf, ls, C, dirt=0xA5)[1:], out[1:])
    fwd = run(z, t8, ls, C, grad=False)
    assert fwd[0] == 0 and same((fwd[1], fwd[4]), (loss, prob)) and fwd[2].isnan() and fwd[3].isnan().all()
    if ls == 0.0:
        null = run(z, t8, None, C)
        assert null[0] == 0 and same((null[1], *null[3:]), (loss, dz, prob)) and null[2].isnan()
    if B == 5:
        strip = run(z, t8, ls, C, row0=3, nrows=2)
        assert strip[0] == 0 and same(strip[3:], out[3:], slice(3, 5)) and strip[3][:3].isnan().all() and strip[4][:3].isnan().all()
    for bad in (dict(ldz=C - 1), dict(kind=2), dict(nrows=B + 1), dict(row0=-1)):      # VIPANT_EBADSHAPE, and nothing is written
        rc, *outs = run(z, t8, ls, C, **bad)
        assert rc == -1 and all(o.isnan().all() for o in outs), bad


def head_ref(sd, x, t, emulate):
    # float64 restatement of the reference head; `emulate`: bf16 operands where the HIP path has them (tests/test_cls_gpu.py: ref_head)
    rf, rg = (_RoundFwd.apply, _RoundBwd.apply) if emulate else ((lambda v: v), (lambda v: v))
    P = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    h = x = x.double().requires_grad_()
    for i in (0, 2):
        h = rf(F.layer_norm(h, (h.shape[1],), P[f"linear.{i}.weight"], P[f"linear.{i}.bias"], 1e-5)) @ rf(P[f"linear.{i + 1}.weight"]).t()
        h = rg(h + P[f"linear.{i + 1}.bias"] if f"linear.{i + 1}.bias" in P else h)
    logits = P["logit_scale"].exp() * h
    loss = margin_loss(torch.sigmoid(logits), t)
    loss.backward()
    return loss.detach(), dict({k: p.grad for k, p in P.items()}, dx=x.grad), logits.detach()


def test_head_against_the_reference_restatement():
    B, E, C = 64, 512, 527
    cfg = {"name": "BCHingeLossHead", "embed_dim": E, "width": 768, "layers": [256], "scaling": True, "bias": False}
    torch.manual_seed(3)
    head = M.build_loss_head(to_config(cfg), output_dim=C)
    x, t = torch.randn(B, E), (torch.rand(B, C) < 2.7 / C).long()          # AudioSet's density: 2.7 labels a clip
    exact, emu = head_ref(head.state_dict(), x, t, False), head_ref(head.state_dict(), x, t, True)
    head = head.to(DEV).train()
    xd = x.to(DEV).requires_grad_()
    loss = head(xd, t.to(DEV))
    loss.backward()
    loss = float(loss.detach())
    print(f"[hinge head] loss hip {loss:.6f} fp64 {float(exact[0]):.6f} bf16-emulation {float(emu[0]):.6f}")
    assert abs(loss - float(exact[0])) <= 1e-3
    for k, g in dict({k: p.grad for k, p in head.named_parameters()}, dx=xd.grad).items():
        e_hip, e_emu = rel(g, exact[1][k]), rel(emu[1][k], exact[1][k])
        print(f"  {k}: rel err hip {e_hip:.3e} bf16-emulation {e_emu:.3e}")
        assert e_hip <= 1.5 * e_emu + 1e-3, (k, e_hip, e_emu)
    with torch.no_grad():
        assert float(head.eval()(x.to(DEV), t.to(DEV))) == loss
    scores, gold = head.x1s[0], head.x2s[0]
    err = float((scores.cpu().double() - torch.sigmoid(emu[2])).abs().max())
    print(f"  cached scores: largest difference {err:.3e}")
    assert err <= 2e-3 and torch.equal(gold.cpu(), t)
    bce = M.build_loss_head(to_config(dict(cfg, name="BCELossHead")), output_dim=C)
    bce.audios = bce.x1s = bce.x2s = bce.ids = None
    assert head.report() == bce.report(x1s=scores, x2s=gold) and not hasattr(head, "x1s")
