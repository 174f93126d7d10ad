"""vipant_label_nce_fwd_bwd through the C ABI against a float64 restatement of include/vipant_hip.h (bounds: `close` of tests/test_sigmoid_loss_gpu.py).
Sizes sit around the kernels' edges (16-row query blocks, 32-key steps, 128-key wave rounds; E = 640 / 1024: two E-chunks, 576: a ragged one)."""
import contextlib
import math

import pytest
import torch

from test_sigmoid_loss_gpu import SENT, close
from vipant_amd import _ffi

pytestmark = pytest.mark.gpu
BS = (1, 2, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257)


def reference(x1, x2, groups, ls, smax=0.0, row0=0, nrows=None, emulate=False):
    x1, x2 = x1.double(), x2.double()
    B = x1.shape[0]
    rows = slice(row0, row0 + (B if nrows is None else nrows))
    raw = torch.as_tensor(ls, dtype=torch.float64).exp()            # ls: a float or a float64 tensor (differentiable)
    clamped = smax > 0 and float(raw) > smax
    s = smax if clamped else raw
    z = s * (x1 @ x2.t())
    P = torch.eye(B, dtype=torch.bool, device=x1.device)
    if groups is not None:
        g = groups.to(x1.device).long()
        P = P | ((g[:, None] == g[None, :]) & (g[:, None] >= 0))
    n = (P := P.double()).sum(1)
    rl, cl = torch.logsumexp(z, 1), torch.logsumexp(z, 0)
    G = ((z - rl[:, None]).exp() + (z - cl[None, :]).exp() - 2 * P / n[:, None]) / B
    g, a, b = (v.bfloat16().double() for v in (G, x1, x2)) if emulate else (G, x1, x2)
    return {"loss": ((rl - (P * z).sum(1) / n).sum() + (cl - (P * z).sum(0) / n).sum()) / B, "dx1": s * g[rows] @ b,
            "dls": torch.zeros(()) if clamped else (G * z).sum(), "dx2": s * g[:, rows].t() @ a}


def run(x1, x2, groups, ls, smax=0.0, row0=0, nrows=None, ws=None, ws_bytes=None, shape=None, refused=False):
    """One call: inputs inside NaN (ids: live-looking) padding, every output between sentinels, the workspace filled with the byte `ws`."""
    B, E = shape or x1.shape
    nrows = B if nrows is None else nrows
    ins = torch.full((2, x1.numel() + 512), float("nan"), device="cuda")
    ins[0, 256:-256], ins[1, 256:-256] = x1.reshape(-1), x2.reshape(-1)
    ids = torch.zeros(x1.shape[0] + 128, dtype=torch.int32, device="cuda")
    if groups is not None:
        ids[64:-64] = groups.to("cuda", torch.int32)
    grads, scal = torch.full((2, nrows * E + 128), SENT, device="cuda"), torch.full((2, 64), SENT, device="cuda")
    need = _ffi.query("vipant_label_nce_workspace_bytes", B, E, nrows) if ws_bytes is None else ws_bytes
    ws = torch.full((need,), 0xFF if ws is None else ws, dtype=torch.uint8, device="cuda")         # dirty, exact size
    par = torch.tensor([ls], dtype=torch.float32, device="cuda")
    args = (ins[0, 256:].data_ptr(), ins[1, 256:].data_ptr(), None if groups is None else ids[64:].data_ptr(), par.data_ptr(), float(smax),
            scal[0, 32:].data_ptr(), grads[0, 64:].data_ptr(), grads[1, 64:].data_ptr(), scal[1, 32:].data_ptr(), 1.0, B, E, row0, nrows,
            ws.data_ptr(), need, None)
    with pytest.raises(_ffi.VipantError) if refused else contextlib.nullcontext():
        _ffi.call("vipant_label_nce_fwd_bwd", *args)
    torch.cuda.synchronize()
    edges = grads if refused else torch.cat([grads[:, :64], grads[:, -64:]], dim=1)      # a refused call writes nothing at all
    assert bool((edges == SENT).all()) and int((scal != SENT).sum()) == (0 if refused else 2)
    return {"loss": scal[0, 32], "dls": scal[1, 32], "dx1": grads[0, 64:-64].view(nrows, E), "dx2": grads[1, 64:-64].view(nrows, E)}


def check(x1, x2, groups, ls, identity=False, **kw):
    got, again = run(x1, x2, groups, ls, **kw), run(x1, x2, groups, ls, ws=0x5A, **kw)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs from dirty workspaces differ in their bits"
    for ids in (groups, None) if identity else (groups,):          # P = I: the float64 InfoNCE formula as well
        ref, emu = reference(x1, x2, ids, ls, **kw), reference(x1, x2, ids, ls, emulate=True, **kw)
        keys = got if x1.shape[0] > 1 else ("loss", "dls")      # B = 1: one logit's soft-max cancels its target, the float64 dx1 / dx2 are 0
        bad = [k for k in keys if not close(k, got[k], ref[k].to(got[k].device), emu[k])]       # exactly: the bound's absolute term, 1e-3
        assert not bad and (x1.shape[0] > 1 or max(float(got[k].abs().max()) for k in ("dx1", "dx2")) <= 1e-3), bad
    return got


def groups_of(kind, B):
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B))
    return {"none": None, "distinct": perm, "one": torch.full((B,), 7), "mod3": perm % 3,
            "mixed": torch.where(perm % 4 == 0, -1 - (perm // 4) % 2, perm % 5)}[kind]        # -1 / -2: "no label", never a group


def features(B, E, groups=None):
    g, unit = torch.Generator().manual_seed(1000 * B + E), lambda t: torch.nn.functional.normalize(t, dim=-1)
    x2 = unit(torch.randn(B, E, generator=g))[slice(None) if groups is None else groups]      # groups: one bit-identical prompt row per group
    return unit(x2 + 0.7 * unit(torch.randn(B, E, generator=g))).cuda(), x2.cuda()


@pytest.mark.parametrize("B,E,row0,nrows,kind",
                         [(B, E, 0, B, k) for B in BS for E in (64, 512, 640) for k in ("mod3", "mixed")]
                         + [(B, 64, 0, B, k) for B in BS for k in ("none", "distinct", "one")]
                         + [(33, E, 0, 33, k) for E in (576, 1024) for k in ("none", "mod3")]
                         + [(B, 512, r, n, "mod3") for B, r, n in ((257, 128, 129), (130, 127, 3), (17, 16, 1))]
                         + [(48, 512, 0, 48, k) for k in ("prompts-10-0", "prompts-100-0", "prompts-100-50")])
def test_against_float64(B, E, row0, nrows, kind):
    """full batches; strips; prompts-scale-smax: rows of x2 within a group bit-identical, saturated at 100, the active clamp gives dls == 0"""
    _, scale, smax = kind.split("-") if "-" in kind else (kind, 10.0, 0.0)
    ids = groups_of("mod3" if "-" in kind else kind, B)
    got = check(*features(B, E, ids if "-" in kind else None), ids, math.log(float(scale)), identity=kind in ("none", "distinct"),
                smax=float(smax), row0=row0, nrows=nrows)
    assert not float(smax) or float(got["dls"]) == 0.0


@pytest.mark.parametrize("B,E,row0,nrows,short", [(8, 96, 0, 8, 0), (8, 1088, 0, 8, 0), (8, 64, 4, 5, 0), (8, 64, 0, 8, 1)])
def test_refusals_write_nothing(B, E, row0, nrows, short):
    run(*features(8, 1088), groups_of("mod3", 8), 0.0, row0=row0, nrows=nrows, shape=(B, E), refused=True,
        ws_bytes=_ffi.query("vipant_label_nce_workspace_bytes", B, E, nrows) - 1 if short else 1 << 20)
