"""vipant_soft_nce_fwd_bwd through the C ABI against a float64 restatement of include/vipant_hip.h (matrices: `close` of
tests/test_sigmoid_loss_gpu.py; scalars: its bound plus the change of the float64 value under c +- 2^-18, the lo.lo term the teacher
product drops).  Sizes sit around the kernels' edges: 16 rows per wave, 64 rows per workgroup = the 64-key tile; 257: five tiles, the
last ragged; E = 576: two E-chunks, the second ragged."""
import contextlib
import math

import pytest
import torch

from test_label_nce_gpu import reference as label_reference
from test_sigmoid_loss_gpu import SENT, close
from vipant_amd import _ffi

pytestmark = pytest.mark.gpu
BS = (1, 2, 15, 16, 17, 63, 64, 65, 257)
CWCL = (-1.0, 1.0)


def reference(x1, x2, t, ls, wf=-1.0, wp=1.0, smax=0.0, row0=0, nrows=None, emulate=False, dc=0.0):
    x1, x2 = x1.double(), x2.double()
    B = x1.shape[0]
    rows = slice(row0, row0 + (B if nrows is None else nrows))
    raw = math.exp(ls)
    clamped = smax > 0 and raw > smax
    s = smax if clamped else raw
    z, eye = s * (x1 @ x2.t()), torch.eye(B, dtype=torch.float64, device=x1.device)
    W = eye if t is None else torch.where(eye > 0, eye, (((t.double() @ t.double().t()) + dc - wf) / (1 - wf)).clamp(0, 1) ** wp)
    n = W.sum(1)
    rl, cl = torch.logsumexp(z, 1), torch.logsumexp(z, 0)
    G = ((z - rl[:, None]).exp() + (z - cl[None, :]).exp() - W * (1 / n[:, None] + 1 / n[None, :])) / B
    g, a, b = (v.bfloat16().double() for v in (G, x1, x2)) if emulate else (G, x1, x2)
    return {"loss": ((rl - (W * z).sum(1) / n).sum() + (cl - (W * z).sum(0) / n).sum()) / B, "dx1": s * g[rows] @ b,
            "dls": torch.zeros((), dtype=torch.float64) if clamped else (G * z).sum(), "dx2": s * g[:, rows].t() @ a}


def run(x1, x2, t, ls, wf=-1.0, wp=1.0, smax=0.0, row0=0, nrows=None, ws=None, short=0, shape=None, refused=False):
    """One call: inputs inside NaN padding, every output between sentinels, the workspace exact-size and filled with the byte `ws`.
    t: None, the string "x2" (the call gets x2's own address) or a tensor [B, Et]; shape: (B, E, Et) the call is told."""
    alias, t = isinstance(t, str), (x2 if isinstance(t, str) else t)
    B, E, Et = shape or (*x1.shape, 0 if t is None else t.shape[1])
    nrows = B if nrows is None else nrows
    pad = lambda v: torch.cat([torch.full((256,), float("nan")), v.reshape(-1).cpu(), torch.full((256,), float("nan"))]).cuda()  # noqa: E731
    p1, p2 = pad(x1), pad(x2)
    pt = p2 if alias else (None if t is None else pad(t))
    grads, scal = torch.full((2, nrows * E + 128), SENT, device="cuda"), torch.full((2, 64), SENT, device="cuda")
    need = max(_ffi.query("vipant_soft_nce_workspace_bytes", B, E, Et, nrows) - short, 1)
    buf = torch.full((need,), 0xFF if ws is None else ws, dtype=torch.uint8, device="cuda")
    par = torch.tensor([ls], dtype=torch.float32, device="cuda")
    args = (p1[256:].data_ptr(), p2[256:].data_ptr(), None if pt is None else pt[256:].data_ptr(), Et, wf, wp, par.data_ptr(), float(smax),
            scal[0, 32:].data_ptr(), grads[0, 64:].data_ptr(), grads[1, 64:].data_ptr(), scal[1, 32:].data_ptr(), 1.0, B, E, row0, nrows,
            buf.data_ptr(), need, None)
    with pytest.raises(_ffi.VipantError) if refused else contextlib.nullcontext():
        _ffi.call("vipant_soft_nce_fwd_bwd", *args)
    torch.cuda.synchronize()
    edges = grads if refused else torch.cat([grads[:, :64], grads[:, -64:]], dim=1)      # a refused call writes nothing at all
    assert bool((edges == SENT).all()) and int((scal != SENT).sum()) == (0 if refused else 2)
    return {"loss": scal[0, 32], "dls": scal[1, 32], "dx1": grads[0, 64:-64].view(nrows, E), "dx2": grads[1, 64:-64].view(nrows, E)}


def scalars_ok(got, want, shifted):
    """loss and dls: `close`'s scalar bound + the larger change of the float64 value `shifted[0]` under c +- 2^-18 (`shifted[1:]`)"""
    bad = []
    for k in ("loss", "dls"):
        extra = max(abs(float(v[k] - shifted[0][k])) for v in shifted[1:])
        err, bound = abs(float(got[k]) - float(want[k])), 5e-5 * abs(float(want[k])) + 1e-6 + extra
        print(f"{k}: {float(got[k]):.8g} ref {float(want[k]):.8g} |err| {err:.2e} = {err / bound:.2f} of the bound (c +- 2^-18: {extra:.2e})")
        bad += [k] * (not (math.isfinite(float(got[k])) and err <= bound))
    return bad


def check(x1, x2, t, ls, refs=(), **kw):
    """refs: further float64 values {loss, dls, dx1, dx2} the call must meet under the same bounds (another formula of the same case)"""
    got, again = run(x1, x2, t, ls, **kw), run(x1, x2, t, ls, ws=0x5A, **kw)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs from dirty workspaces differ in their bits"
    tt = x2 if isinstance(t, str) else t
    ref, emu = reference(x1, x2, tt, ls, **kw), reference(x1, x2, tt, ls, emulate=True, **kw)
    shifted = [ref] + [reference(x1, x2, tt, ls, dc=d, **kw) for d in (2.0 ** -18, -2.0 ** -18) if tt is not None]
    bad = []
    for want in (ref, *refs):
        bad += scalars_ok(got, want, shifted + [ref])
        if x1.shape[0] > 1:     # B = 1: one logit's soft-max cancels its target, the float64 dx1 / dx2 are 0
            bad += [k for k in ("dx1", "dx2") if not close(k, got[k], want[k].to(got[k].device), emu[k])]
    assert not bad and (x1.shape[0] > 1 or max(float(got[k].abs().max()) for k in ("dx1", "dx2")) <= 1e-3), bad
    return got


def features(B, E, Et, groups=None):
    g, unit = torch.Generator().manual_seed(1000 * B + E + Et), lambda v: torch.nn.functional.normalize(v, dim=-1)
    x2 = unit(torch.randn(B, E, generator=g))
    t = unit(x2[:, :Et] + 0.5 * unit(torch.randn(B, Et, generator=g))) if Et <= E else unit(torch.randn(B, Et, generator=g))
    if groups is not None:
        t = t[groups]           # one bit-identical teacher row per group
    return unit(x2 + 0.7 * unit(torch.randn(B, E, generator=g))).cuda(), x2.cuda(), t.cuda()


FULL = ([(B, 64, 64, 0, B, "sep", CWCL, 10, 0) for B in BS] + [(B, 512, 512, 0, B, "x2", (0.0, 1.0), 10, 0) for B in BS]
        + [(B, 64, 64, 0, B, "none", CWCL, 10, 0) for B in (1, 17, 257)]
        + [(33, 576, 576, 0, 33, "sep", (0.5, 4.0), 10, 0), (65, 64, 128, 0, 65, "sep", CWCL, 10, 0), (65, 512, 64, 0, 65, "sep", CWCL, 100, 0)]
        + [(65, 64, 64, 0, 65, k, w, 10, 0) for k in ("x2", "sep") for w in (CWCL, (0.0, 1.0), (0.5, 4.0))]
        + [(B, 512, 512, r, n, "sep", CWCL, 10, 0) for B, r, n in ((257, 128, 129), (130, 127, 3), (17, 16, 1))]
        + [(48, 512, 512, 0, 48, "groups", (0.999, 1.0), s, m) for s, m in ((10, 0), (100, 0), (100, 50))])


@pytest.mark.parametrize("B,E,Et,row0,nrows,kind,w,scale,smax", FULL)
def test_against_float64(B, E, Et, row0, nrows, kind, w, scale, smax):
    """teachers: none (W = I: also InfoNCE's cross-entropy form), x2 (aliased), sep(arate), groups (bit-identical rows inside three
    groups, w_floor = 0.999: also the label-aware formula with those groups); strips; s = 100; the active clamp gives dls == 0"""
    ids = torch.randperm(B, generator=torch.Generator().manual_seed(B)) % 3 if kind == "groups" else None
    x1, x2, t = features(B, E, Et, ids)
    ls, kw, refs = math.log(float(scale)), dict(smax=float(smax), row0=row0, nrows=nrows), ()
    if kind == "groups":
        refs = (label_reference(x1, x2, ids, ls, **kw),)
    if kind == "none":
        z, tgt = float(scale) * (x1.double() @ x2.double().t()), torch.arange(B, device="cuda")
        ce = torch.nn.functional.cross_entropy
        refs = (dict(reference(x1, x2, None, ls, **kw), loss=ce(z, tgt) + ce(z.t(), tgt)),)
    got = check(x1, x2, {"none": None, "x2": "x2"}.get(kind, t), ls, refs=refs, wf=w[0], wp=w[1], **kw)
    assert not smax or float(got["dls"]) == 0.0


@pytest.mark.parametrize("shape,w,row0,nrows,short", [((8, 96, 64), CWCL, 0, 8, 0), ((8, 64, 96), CWCL, 0, 8, 0), ((8, 64, 64), (1.0, 1.0), 0, 8, 0),
                                                      ((8, 64, 64), (-1.0, 0.0), 0, 8, 0), ((8, 64, 64), CWCL, 4, 5, 0), ((8, 64, 64), CWCL, 0, 8, 1)])
def test_refusals_write_nothing(shape, w, row0, nrows, short):
    x1, x2, t = features(8, 128, 128)
    if not short:
        short = -(1 << 20)      # a refused shape's query is 0: any workspace will do
    run(x1, x2, t, 0.0, wf=w[0], wp=w[1], row0=row0, nrows=nrows, shape=shape, short=short, refused=True)
