"""Classification loss heads on the MI355X (model/loss=ce_cls, bce; cvap/module/decoder/loss_head.py:330-419, loss_more.py:29-143).

Kernel level (fp32 logits in): loss, dscale, pred and prob against a float64 restatement within 1e-5 relative (fp32 rounding
only, the bound the Barlow kernels are held to); dz within one bf16 rounding of the float64 value (2^-8 relative + 1e-7).
Head level: against the reference fixtures (tests/golden/make_golden_cls.py): loss within 1e-3, gradients within 1.5 x the error
of a bf16-operand emulation of the head + 1e-3, the emulation computed here (the rule of tests/test_barlow_gpu.py).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
DEV = "cuda:0"
F64 = torch.float64
LS0 = float(np.log(1 / 0.07))


@pytest.fixture(scope="module")
def ops():
    from vipant_amd import _ffi, ops as O
    _ffi.call("vipant_device_check")
    return O


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bf16_close(got, ref, what):
    """bf16 output against fp64: one bf16 rounding (2^-8 relative) + 1e-7."""
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    bad = err > 2.0 ** -8 * ref.abs() + 1e-7
    assert not bad.any(), (what, int(bad.sum()), float(err.max()))


def close(a, b, what, tol=1e-5):
    a, b = float(a), float(b)
    print(f"  {what}: hip {a:.9g} fp64 {b:.9g}")
    assert abs(a - b) <= tol * abs(b), (what, a, b)


def pad(z, ld):
    out = torch.full((z.shape[0], ld), 7.0)           # the pad of z is never read: poison it
    out[:, :z.shape[1]] = z
    return out


def ce_ref(z, y, ls):
    z = z.double().requires_grad_()
    lsd = torch.tensor(ls, dtype=F64, requires_grad=True)
    loss = F.cross_entropy(lsd.exp() * z, y)
    loss.backward()
    return loss.detach(), z.grad, lsd.grad


def bce_ref(z, t, ls):
    z = z.double().requires_grad_()
    lsd = torch.tensor(0.0 if ls is None else ls, dtype=F64, requires_grad=ls is not None)
    x = lsd.exp() * z
    loss = F.binary_cross_entropy_with_logits(x, t.double())
    loss.backward()
    return loss.detach(), z.grad, lsd.grad, torch.sigmoid(x.detach())


SHAPES = [(B, C) for B in (1, 50, 128, 1000) for C in (10, 50, 64, 527)]


@pytest.mark.parametrize("B,C", SHAPES)
def test_softmax_ce_kernel_against_fp64(ops, B, C):
    ld = (C + 63) // 64 * 64
    z = rnd(B, C, scale=0.5, seed=B + C)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(C))
    y[::3] = z[::3].argmax(-1)                        # confident, correct rows: 1 - p is tiny there
    ls = torch.tensor(LS0)
    loss, dz, dls, pred = ops.softmax_ce(pad(z, ld).to(DEV), y.to(DEV), ls.to(DEV), C=C, ldd=ld)
    rl, rdz, rdls = ce_ref(z, y, LS0)
    print(f"[softmax_ce B={B} C={C}]")
    close(loss, rl, "loss")
    close(dls, rdls, "dscale")
    bf16_close(dz[:, :C], rdz, "dz")
    assert not dz[:, C:].any(), "pad columns of dz must be zero"
    assert torch.equal(pred.cpu().long(), z.argmax(-1))


@pytest.mark.parametrize("B,C", SHAPES)
def test_bce_logits_kernel_against_fp64(ops, B, C):
    ld = (C + 63) // 64 * 64
    z = rnd(B, C, scale=0.3, seed=2 * B + C)
    t = (torch.rand(B, C, generator=torch.Generator().manual_seed(B)) < 0.1).to(torch.uint8)
    for ls in (LS0, None):
        lst = None if ls is None else torch.tensor(ls).to(DEV)
        loss, dz, dls, prob = ops.bce_logits(pad(z, ld).to(DEV), t.to(DEV), lst, C=C, ldd=ld, want_prob=True)
        rl, rdz, rdls, rp = bce_ref(z, t, ls)
        print(f"[bce_logits B={B} C={C} scaling={ls is not None}]")
        close(loss, rl, "loss")
        if ls is not None:
            close(dls, rdls, "dscale")
        else:
            assert dls is None
        bf16_close(dz[:, :C], rdz, "dz")
        assert not dz[:, C:].any()
        perr = float(((prob.cpu().double() - rp).abs() / rp).max())
        assert perr <= 1e-5, perr


def test_wide_rows_take_the_streaming_kernel(ops):
    """C > 1024: the row no longer fits the registers of one wave and is read from memory in every pass."""
    B, C = 33, 1500
    z = rnd(B, C, scale=0.4, seed=9)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(1))
    loss, dz, dls, pred = ops.softmax_ce(z.to(DEV), y.to(DEV), torch.tensor(LS0).to(DEV), ldd=1536)
    rl, rdz, rdls = ce_ref(z, y, LS0)
    close(loss, rl, "loss"); close(dls, rdls, "dscale")
    bf16_close(dz[:, :C], rdz, "dz")
    assert not dz[:, C:].any() and torch.equal(pred.cpu().long(), z.argmax(-1))


def test_argmax_takes_the_first_index_on_exact_ties(ops):
    z = torch.zeros(6, 50)
    z[0, [7, 3, 49]] = 2.0
    z[1, [48, 49]] = 1.0
    z[2] = -1.0
    z[3, 0] = 5.0
    z[4, [20, 21]] = 3.0
    y = torch.zeros(6, dtype=torch.int64)
    _, _, _, pred = ops.softmax_ce(z.to(DEV), y.to(DEV), torch.tensor(0.0).to(DEV), want_grad=False)
    assert pred.cpu().tolist() == z.argmax(-1).tolist() == [3, 48, 0, 0, 20, 0]


def test_large_logits_stay_finite(ops):
    """Scaled logits of +-80: exp() of either sign must not overflow a loss or a gradient."""
    B, C = 64, 50
    z = rnd(B, C, seed=3).sign() * 80.0 * torch.rand(B, C, generator=torch.Generator().manual_seed(4))
    z[:, 0], z[:, 1] = 80.0, -80.0
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(5))
    zero = torch.tensor(0.0).to(DEV)
    loss, dz, dls, _ = ops.softmax_ce(z.to(DEV), y.to(DEV), zero)
    rl, rdz, rdls = ce_ref(z, y, 0.0)
    assert torch.isfinite(loss).all() and torch.isfinite(dz.float()).all() and torch.isfinite(dls).all()
    close(loss, rl, "ce loss"); close(dls, rdls, "ce dscale"); bf16_close(dz, rdz, "ce dz")
    t = (z > 0).to(torch.uint8)
    t[::2] = 1 - t[::2]
    loss, dz, dls, prob = ops.bce_logits(z.to(DEV), t.to(DEV), zero, want_prob=True)
    rl, rdz, rdls, rp = bce_ref(z, t, 0.0)
    assert torch.isfinite(loss).all() and torch.isfinite(dz.float()).all() and torch.isfinite(prob).all()
    close(loss, rl, "bce loss"); close(dls, rdls, "bce dscale"); bf16_close(dz, rdz, "bce dz")


def test_row_slices_sum_to_the_whole_and_runs_are_bit_identical(ops):
    B, C, ld = 103, 50, 64
    z = pad(rnd(B, C, scale=0.5, seed=11), ld).to(DEV)
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(12)).to(DEV)
    t = (torch.rand(B, C, generator=torch.Generator().manual_seed(13)) < 0.2).to(torch.uint8).to(DEV)
    ls = torch.tensor(LS0).to(DEV)
    for name, fn, tgt in (("ce", ops.softmax_ce, y), ("bce", ops.bce_logits, t)):
        whole = fn(z, tgt, ls, C=C, ldd=ld)
        again = fn(z, tgt, ls, C=C, ldd=ld)
        assert all(torch.equal(a, b) for a, b in zip(whole[:3], again[:3])), name
        cuts = [(0, 40), (40, 1), (41, 62)]
        parts = [fn(z, tgt, ls, C=C, ldd=ld, row0=r0, nrows=n, grad_scale=0.5) for r0, n in cuts]
        close(sum(float(p[0]) for p in parts), whole[0], f"{name} loss of the slices")
        close(2.0 * sum(float(p[2]) for p in parts), whole[2], f"{name} dscale of the slices")
        for (r0, n), p in zip(cuts, parts):
            bf16_close(2.0 * p[1][r0:r0 + n].float(), whole[1][r0:r0 + n].float(), f"{name} dz rows {r0}+{n}")


def test_bad_arguments_are_reported(ops):
    from vipant_amd._ffi import VipantError
    z = torch.zeros(8, 64, device=DEV)
    y = torch.zeros(8, dtype=torch.int64, device=DEV)
    ls = torch.zeros((), device=DEV)
    with pytest.raises(VipantError, match="row range"):
        ops.softmax_ce(z, y, ls, C=50, row0=4, nrows=8)
    with pytest.raises(VipantError, match="ldd"):
        ops.softmax_ce(z, y, ls, C=50, ldd=48)
    with pytest.raises(VipantError, match="bad shape"):
        ops.softmax_ce(z, y, ls, C=65)
    loss, dz, _, pred = ops.softmax_ce(z, y + 1000, ls, C=50)            # an out-of-range label is clamped, never dereferenced
    assert torch.isfinite(loss).all() and int(pred.max()) == 0


# ------------------------------------------------------------------------------------------------ heads against the reference
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


def ref_head(sd, kind, x, target, scaling, emulate):
    """float64 restatement of the head's training forward; with `emulate` the values are rounded to bf16 where the HIP path
    rounds them: LayerNorm outputs, weights, and the gradient of every Linear's output."""
    rf = _RoundFwd.apply if emulate else (lambda t: t)
    rg = _RoundBwd.apply if emulate else (lambda t: t)
    P = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    x = x.double().requires_grad_()
    h = x
    n = max(int(k.split(".")[1]) for k in P if k.startswith("linear.")) + 1
    for i in range(0, n, 2):
        h = rf(F.layer_norm(h, (h.shape[1],), P[f"linear.{i}.weight"], P[f"linear.{i}.bias"], 1e-5))
        h = h @ rf(P[f"linear.{i + 1}.weight"]).t()
        if f"linear.{i + 1}.bias" in P:
            h = h + P[f"linear.{i + 1}.bias"]
        h = rg(h)
    scale = P["logit_scale"].exp() if "logit_scale" in P else 1.0
    loss = F.cross_entropy(scale * h, target) if kind == "ce" else F.binary_cross_entropy_with_logits(scale * h, target.double())
    loss.backward()
    return loss.detach(), P, x


def build(tag):
    import gen_cls
    import vipant_amd.module as M
    from vipant_amd.config import to_config
    kind, B, C, layers, bias, scaling, n = gen_cls.CASES[tag]
    cfg = ({"name": "ClassificationHead", "embed_dim": 512, "layers": [], "scaling": True} if kind == "ce" else
           {"name": "BCELossHead", "embed_dim": 512, "width": 768, "layers": layers, "scaling": scaling, "bias": bias})
    head = M.build_loss_head(to_config(cfg), output_dim=C)
    head.load_state_dict(dict(head.state_dict(), **gen_cls.head_weights(tag, head.state_dict(), C)), strict=True)
    x, y = (gen_cls.ce_inputs if kind == "ce" else gen_cls.bce_inputs)(tag, B, C)
    return head, x, y, kind, scaling


def rel(a, b):
    a, b = a.double().cpu().reshape(-1), b.double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def fixture_grad(fx, k, got):
    """(what the HIP path has, what the reference has) for gradient k: in full, or at the fixture's sampled positions."""
    if f"g_{k}" in fx:
        return got.reshape(-1), torch.from_numpy(fx[f"g_{k}"]).reshape(-1)
    return got.reshape(-1)[torch.from_numpy(fx[f"idx_{k}"])], torch.from_numpy(fx[f"s_{k}"])


@pytest.mark.parametrize("tag", ["cls_esc50", "cls_us8k", "bce_as", "bce_hidden"])
def test_head_against_the_reference_fixture(tag):
    fx = np.load(os.path.join(GOLD, tag + ".npz"))
    head, x, y, kind, scaling = build(tag)
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    head = head.to(DEV).train()
    xd = x.to(DEV).requires_grad_()
    loss = head(xd, y.to(DEV))
    loss.backward()
    ref = ref_head(sd, kind, x, y, scaling, emulate=False)
    emu = ref_head(sd, kind, x, y, scaling, emulate=True)
    print(f"[{tag}] loss hip {float(loss):.6f} reference {float(fx['loss']):.6f} fp64 {float(ref[0]):.6f} "
          f"bf16-emulation {float(emu[0]):.6f}")
    assert abs(float(ref[0]) - float(fx["loss"])) <= 1e-4, "the restatement is not the reference"
    assert abs(float(loss) - float(fx["loss"])) <= 1e-3, (float(loss), float(fx["loss"]))
    got = {k: p.grad for k, p in head.named_parameters()}
    got["dx"] = xd.grad
    exact = {k: p.grad for k, p in ref[1].items()}
    exact["dx"] = ref[2].grad
    emul = {k: p.grad for k, p in emu[1].items()}
    emul["dx"] = emu[2].grad
    for k, g in got.items():
        assert g is not None, k
        mine, theirs = fixture_grad(fx, k, g.detach().cpu())
        e_hip, e_emu = rel(mine, theirs), rel(emul[k], exact[k])
        print(f"  {k}: rel err hip {e_hip:.3e} bf16-emulation {e_emu:.3e}")
        assert rel(exact[k] if f"g_{k}" in fx else exact[k].reshape(-1)[torch.from_numpy(fx[f"idx_{k}"])], theirs) <= 1e-4, k
        assert e_hip <= 1.5 * e_emu + 1e-3, (k, e_hip, e_emu)


def test_head_is_bit_identical_run_to_run():
    head, x, y, _, _ = build("cls_esc50")
    head = head.to(DEV).train()
    runs = []
    for _ in range(2):
        head.zero_grad(set_to_none=True)
        loss = head(x.to(DEV), y.to(DEV))
        loss.backward()
        runs.append([loss.detach().clone()] + [p.grad.clone() for p in head.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_bce_eval_scores_and_loss_against_the_reference():
    import gen_cls
    fx = np.load(os.path.join(GOLD, "cls_reports.npz"))
    q = np.concatenate([np.load(os.path.join(GOLD, f"bce_scores{i}.npz"))["scores"] for i in (0, 1)]).astype(np.float64)
    head, _, _, _, _ = build("bce_as")
    head = head.to(DEV).eval()
    x, Y = gen_cls.bce_inputs("bce_as", 1054, 527, part="eval")
    with torch.no_grad():
        losses = [float(head(x[i:i + 527].to(DEV), Y[i:i + 527].to(DEV))) for i in range(0, 1054, 527)]
    scores = torch.cat(head.x1s).cpu().double().numpy()
    # scaled logits reach 30 and carry the bf16 operands' error (about 0.05, see cls_reports); d sigmoid <= 1 / 4, and the
    # stored scores are fp16: |d score| <= 0.25 x 4 x 0.05 + 2^-11
    err = np.abs(scores - q).max()
    print(f"[bce eval] largest score difference {err:.3e}; losses hip {losses} reference {fx['loss_bce_as_eval'].tolist()}")
    assert err <= 0.05 + 2.0 ** -11, err
    assert np.abs(np.array(losses) - fx["loss_bce_as_eval"]).max() <= 1e-3
    report = head.report()
    assert report.startswith("Mac-AP = ") and report.endswith("@ 1054") and "Err(False)" in report, report
    assert not hasattr(head, "x1s")
