"""Soft-target binary cross entropy (vipant_bce_logits_soft, ops.bce_logits_soft) on the MI355X against float64.

Bounds are the kernel family's (tests/test_cls_gpu.py): loss and dscale within 1e-5 relative (fp32 rounding
only), dz within one bf16 rounding of the float64 value (2^-8 relative + 1e-7).  Targets are uniform in [0, 1] with exact 0s and
1s mixed in -- those elements take the binary kernel's arithmetic -- and the scaled logits reach +-30.  On float {0, 1} targets
every output equals ops.bce_logits on the uint8 form bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
LS0 = float(np.log(1 / 0.07))
# tests/test_cls_gpu.py's BCE cases, (1, 10) among them, and (5, 1100): rows wider than the soft-max kernels keep in registers, padded ldd
SHAPES = [(B, C) for B in (1, 50, 128, 1000) for C in (10, 50, 64, 527)] + [(5, 1100)]


@pytest.fixture(scope="module")
def ops():
    from vipant_amd import _ffi, ops as O
    _ffi.call("vipant_device_check")
    return O


def bf16_close(got, ref, what):
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


def inputs(B, C, ls):
    """z with scaled logits uniform in [-30, 30]; targets uniform in [0, 1], a fifth exactly 0 and a fifth exactly 1."""
    g = torch.Generator().manual_seed(7 * B + C)
    s = 1.0 if ls is None else float(np.exp(ls))
    z = (60.0 * torch.rand(B, C, generator=g) - 30.0) / s
    z.view(-1)[0], z.view(-1)[-1] = 30.0 / s, -30.0 / s
    t = torch.rand(B, C, generator=g)
    pick = torch.rand(B, C, generator=g)
    t[pick < 0.2] = 0.0
    t[pick > 0.8] = 1.0
    return z, t


def bce_ref(z, t, ls):
    z = z.double().requires_grad_()
    lsd = torch.tensor(0.0 if ls is None else ls, dtype=F64, requires_grad=ls is not None)
    x = lsd.exp() * z
    loss = F.binary_cross_entropy_with_logits(x, t.double())
    loss.backward()
    return loss.detach(), z.grad, lsd.grad, torch.sigmoid(x.detach())


@pytest.mark.parametrize("B,C", SHAPES)
def test_soft_kernel_against_fp64(ops, B, C):
    ld = (C + 63) // 64 * 64
    for ls in (LS0, None):
        z, t = inputs(B, C, ls)
        lst = None if ls is None else torch.tensor(ls).to(DEV)
        loss, dz, dls, prob = ops.bce_logits_soft(pad(z, ld).to(DEV), t.to(DEV), lst, C=C, ldd=ld, want_prob=True)
        rl, rdz, rdls, rp = bce_ref(z, t, ls)
        print(f"[bce_logits_soft B={B} C={C} scaling={ls is not None}]")
        close(loss, rl, "loss")
        if ls is not None:
            close(dls, rdls, "dscale")
        else:
            assert dls is None
        bf16_close(dz[:, :C], rdz, "dz")
        assert dz.shape == (B, ld) and not dz[:, C:].any()
        assert torch.isfinite(prob).all()
        perr = float((prob.cpu().double() - rp).abs().max())
        assert perr <= 1e-6, perr                         # absolute: sigmoid(-30) is 1e-13


@pytest.mark.parametrize("B,C", [(1, 10), (50, 527), (5, 1100)])
def test_binary_float_targets_give_the_binary_kernels_bits(ops, B, C):
    ld = (C + 63) // 64 * 64
    for ls in (LS0, None):
        z, t = inputs(B, C, ls)
        t8 = (t > 0.5).to(torch.uint8)
        lst = None if ls is None else torch.tensor(ls).to(DEV)
        zd = pad(z, ld).to(DEV)
        soft = ops.bce_logits_soft(zd, t8.float().to(DEV), lst, C=C, ldd=ld, want_prob=True)
        hard = ops.bce_logits(zd, t8.to(DEV), lst, C=C, ldd=ld, want_prob=True)
        for name, a, b in zip(("loss", "dz", "dscale", "prob"), soft, hard):
            assert (a is None and b is None) or torch.equal(a, b), name


def test_row_slices_sum_to_the_whole_and_runs_are_bit_identical(ops):
    B, C, ld = 103, 50, 64
    z, t = inputs(B, C, LS0)
    z, t, ls = pad(z, ld).to(DEV), t.to(DEV), torch.tensor(LS0).to(DEV)
    whole = ops.bce_logits_soft(z, t, ls, C=C, ldd=ld)
    again = ops.bce_logits_soft(z, t, ls, C=C, ldd=ld)
    assert all(torch.equal(a, b) for a, b in zip(whole[:3], again[:3]))
    cuts = [(0, 40), (40, 1), (41, 62)]
    parts = [ops.bce_logits_soft(z, t, ls, C=C, ldd=ld, row0=r0, nrows=n, grad_scale=0.5) for r0, n in cuts]
    close(sum(float(p[0]) for p in parts), whole[0], "loss of the slices")
    close(2.0 * sum(float(p[2]) for p in parts), whole[2], "dscale of the slices")
    for (r0, n), p in zip(cuts, parts):
        bf16_close(2.0 * p[1][r0:r0 + n].float(), whole[1][r0:r0 + n].float(), f"dz rows {r0}+{n}")


def test_bad_arguments_are_refused(ops):
    from vipant_amd import _ffi
    z = torch.zeros(8, 64, device=DEV)
    t = torch.full((8, 64), 0.5, device=DEV)
    ws = ops.scratch("classify", _ffi.query("vipant_bce_logits_workspace_bytes", 8), z.device)
    loss = torch.full((1,), -7.0, device=DEV)
    dscale = torch.full((1,), -7.0, device=DEV)
    # dscale without logit_scale is refused, and nothing is written
    rc = _ffi.lib().vipant_bce_logits_soft(z.data_ptr(), 64, t.data_ptr(), 64, None, loss.data_ptr(), None, 64, dscale.data_ptr(), None,
                                           64, 0, 8, 1.0, 8, 50, ws.data_ptr(), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and float(loss) == -7.0 and float(dscale) == -7.0
    assert b"dscale needs logit_scale" in _ffi.lib().vipant_last_error()
    with pytest.raises(_ffi.VipantError, match="row range"):
        ops.bce_logits_soft(z, t, None, C=50, row0=4, nrows=8)
    with pytest.raises(_ffi.VipantError, match="ldd"):
        ops.bce_logits_soft(z, t, None, C=50, ldd=48)
    with pytest.raises(Exception):
        ops.bce_logits_soft(z, t.to(torch.uint8), None, C=50)              # the soft entry point takes fp32 targets only
    assert ops.bce_logits_soft(z, t, None, C=50)[2] is None                 # logit_scale None: no dscale is produced


def test_classifier_fn_takes_the_soft_kind(ops):
    """ClassifierMeta(kind="bce_soft") through ClassifierFn: half-integer targets change dz, the backward contractions are shared."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(16, 256, generator=g).to(DEV)
    params = [torch.ones(256), torch.zeros(256), 0.05 * torch.randn(12, 256, generator=g), None]
    y = (torch.rand(16, 12, generator=g) < 0.3).float()
    out = {}
    for kind, tgt in (("bce", y.to(torch.uint8)), ("bce_soft", y), ("half", 0.5 * y)):
        ps = [None if p is None else p.clone().to(DEV).requires_grad_() for p in params]
        meta = ops.ClassifierMeta("bce_soft" if kind == "half" else kind, 12)
        loss = ops.ClassifierFn.apply(x, tgt.to(DEV), torch.zeros((), device=DEV), meta, *ps)
        loss.backward()
        out[kind] = (loss.detach(), ps[2].grad)
    assert torch.equal(out["bce"][0], out["bce_soft"][0]) and torch.equal(out["bce"][1], out["bce_soft"][1])
    assert not torch.equal(out["bce"][1], out["half"][1])
