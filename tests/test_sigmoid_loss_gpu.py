"""vipant_sigmoid_loss_fwd_bwd through the C ABI against a float64 restatement of include/vipant_hip.h.  Sizes sit on either side of the
kernel's edges (16-row query blocks, 32-key steps, the waves' round of 128 keys; E = 640 / 1024: two full E-chunks, 576: a ragged one)."""
import contextlib
import math

import pytest
import torch

from vipant_amd import _ffi

pytestmark = pytest.mark.gpu
SENT = -777.25


def reference(x1, x2, ls, lb, smax=0.0, row0=0, nrows=None, emulate=False):
    x1, x2 = x1.double(), x2.double()
    B = x1.shape[0]
    rows = slice(row0, row0 + (B if nrows is None else nrows))
    raw = torch.as_tensor(ls, dtype=torch.float64).exp()            # ls, lb: floats or float64 tensors (differentiable)
    clamped = smax > 0 and float(raw) > smax
    s = smax if clamped else raw
    d = x1 @ x2.t()
    y = 2 * torch.eye(B, dtype=torch.float64, device=x1.device) - 1
    u = -y * (s * d + lb)
    G = -y * torch.sigmoid(u) / B
    g, a, b = (v.bfloat16().double() for v in (G, x1, x2)) if emulate else (G, x1, x2)
    return {"loss": torch.logaddexp(u, torch.zeros_like(u))[rows].sum() / B, "dlb": G[rows].sum(), "dx1": s * g[rows] @ b,
            "dls": torch.zeros(()) if clamped else s * (G[rows] * d[rows]).sum(), "dx2": s * g[:, rows].t() @ a}


def close(name, got, ref, emu):
    # scalars: the InfoNCE kernel's bound; matrices: rel-L2 and max-abs <= 1.5 x the error of `emu` (bf16 G and operand in float64) + 1e-3
    got, err = got.double(), lambda a, f: float(f(a - ref) / f(ref))
    if ref.dim() == 0:
        print(f"{name}: {float(got):.8g} ref {float(ref):.8g}")
        return bool(torch.isfinite(got)) and abs(float(got - ref)) <= 5e-5 * abs(float(ref)) + 1e-6
    l2, l2e, mx, mxe = err(got, torch.norm), err(emu, torch.norm), err(got, lambda v: v.abs().max()), err(emu, lambda v: v.abs().max())
    print(f"{name}: rel-L2 {l2:.2e} (emulation {l2e:.2e}) max-abs {mx:.2e} (emulation {mxe:.2e})")
    return bool(torch.isfinite(got).all()) and l2 <= 1.5 * l2e + 1e-3 and mx <= 1.5 * mxe + 1e-3


def run(x1, x2, ls, lb, smax=0.0, row0=0, nrows=None, ws=None, ws_bytes=None, shape=None, refused=False):
    """One call: inputs inside NaN padding, every output between sentinels, the workspace filled with the byte `ws`."""
    B, E = shape or x1.shape
    nrows = B if nrows is None else nrows
    ins = torch.full((2, x1.numel() + 512), float("nan"), device="cuda")
    ins[0, 256:-256], ins[1, 256:-256] = x1.reshape(-1), x2.reshape(-1)
    grads, scal = torch.full((2, nrows * E + 128), SENT, device="cuda"), torch.full((3, 64), SENT, device="cuda")
    need = _ffi.query("vipant_sigmoid_loss_workspace_bytes", B, E, nrows) if ws_bytes is None else ws_bytes
    ws = torch.full((need,), 0xFF if ws is None else ws, dtype=torch.uint8, device="cuda")         # dirty, exact size
    par = torch.tensor([ls, lb], dtype=torch.float32, device="cuda")
    args = (ins[0, 256:].data_ptr(), ins[1, 256:].data_ptr(), par.data_ptr(), par.data_ptr() + 4, float(smax), scal[0, 32:].data_ptr(),
            grads[0, 64:].data_ptr(), grads[1, 64:].data_ptr(), scal[1, 32:].data_ptr(), scal[2, 32:].data_ptr(), 1.0, B, E, row0, nrows,
            ws.data_ptr(), need, None)
    with pytest.raises(_ffi.VipantError) if refused else contextlib.nullcontext():
        _ffi.call("vipant_sigmoid_loss_fwd_bwd", *args)
    torch.cuda.synchronize()
    edges = grads if refused else torch.cat([grads[:, :64], grads[:, -64:]], dim=1)      # a refused call writes nothing at all
    assert bool((edges == SENT).all()) and int((scal != SENT).sum()) == (0 if refused else 3)
    return {"loss": scal[0, 32], "dls": scal[1, 32], "dlb": scal[2, 32], "dx1": grads[0, 64:-64].view(nrows, E),
            "dx2": grads[1, 64:-64].view(nrows, E)}


def check(x1, x2, ls, lb, **kw):
    got, again = run(x1, x2, ls, lb, **kw), run(x1, x2, ls, lb, ws=0x5A, **kw)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs from dirty workspaces differ in their bits"
    ref, emu = reference(x1, x2, ls, lb, **kw), reference(x1, x2, ls, lb, emulate=True, **kw)
    bad = [k for k in got if not close(k, got[k], ref[k].to(got[k].device), emu[k])]
    assert not bad, bad
    return got


def features(B, E, hard=False):
    g, unit = torch.Generator().manual_seed(1000 * B + E), lambda t: torch.nn.functional.normalize(t, dim=-1)
    x1 = unit(torch.randn(B, E, generator=g))
    x2 = unit(x1 + 0.7 * unit(torch.randn(B, E, generator=g)))
    if hard:        # duplicate rows (off-diagonal cosines of +1) and one exactly opposite pair (-1)
        x1[5], x2[3], x2[5], x2[7] = x1[3], x1[3], x1[3], -x1[7]
    return x1.cuda(), x2.cuda()


@pytest.mark.parametrize("B,E,row0,nrows,scale,lb,smax",
                         [(B, E, 0, B, 10.0, -10.0, 0.0) for B in (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257) for E in (64, 512, 640)]
                         + [(B, E, r, n, 10.0, -10.0, 0.0) for B, E, r, n in ((33, 576, 0, 33), (33, 1024, 0, 33), (257, 512, 128, 129), (130, 512, 127, 3), (17, 512, 16, 1))]
                         + [(24, 512, 0, 24, 100.0, lb, smax) for lb, smax in ((-10.0, 0.0), (0.0, 0.0), (10.0, 0.0), (-10.0, 50.0))])
def test_against_float64(B, E, row0, nrows, scale, lb, smax):
    """full batches; strips (dx1 / dx2 the strip's rows, the scalars the sums over the strip's rows: the header's convention); saturated
    logits of +-100 at scale 100, once with the clamp active, which must give dlogit_scale == 0"""
    got = check(*features(B, E, hard=scale == 100.0), math.log(scale), lb, smax=smax, row0=row0, nrows=nrows)
    assert not smax or float(got["dls"]) == 0.0


@pytest.mark.parametrize("B,E,row0,nrows,short", [(8, 96, 0, 8, 0), (8, 1088, 0, 8, 0), (8, 64, 4, 5, 0), (8, 64, 0, 8, 1)])
def test_refusals_write_nothing(B, E, row0, nrows, short):
    ws_bytes = _ffi.query("vipant_sigmoid_loss_workspace_bytes", B, E, nrows) - 1 if short else 1 << 20
    run(*features(8, 1088), 0.0, 0.0, row0=row0, nrows=nrows, ws_bytes=ws_bytes, shape=(B, E), refused=True)
