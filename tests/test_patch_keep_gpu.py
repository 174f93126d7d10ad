"""The kept-patch embedding (patchout; csrc/patch_keep.hip) through the C ABI against plain float64 on the CPU: unfold, gather, matmul on
the bf16-rounded x and the w_eff the operator returned; inputs in NaN guard zones, outputs between sentinels (tests/guards.py).  The bounds
are the issue's: exact operands bit for bit, Gaussian ones within kcols x 2^-23 x (|A| |B|^T + |pos|), dcls / dpos within b x 2^-24 x
sum |terms|, everything else bit for bit against the stand-alone entry points.  The issue's three geometries have at most 28 patches;
the fourth (P = 120) is there for k = 63, 64, 65: a second, ragged row tile."""
import pytest
import torch
import torch.nn.functional as Fn

from guards import FILL, Guarded, Workspace
from vipant_amd import _ffi as ffi, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16, I32, F64 = torch.float32, torch.bfloat16, torch.int32, torch.float64
B = 3
GEOS = [(80, 48, 16, 10), (96, 64, 32, 16), (40, 16, 16, 16), (104, 88, 16, 8)]        # T, F, ph = pw, stride
CASES = [(g, C, D) for g in GEOS for C in (1, 3) for D in (192, 320, 768)]


def bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def nan_guarded(t):
    return Guarded(tuple(t.shape), t.dtype, DEV, init=t.to(DEV), fill=float("nan")).v


def keep_lists(ops, nrow, ncol, seed):
    # [(k, keep int32 [B, k])]: drawn lists at every k of the issue that P allows, one shared set, one disjoint family
    P = nrow * ncol
    g = torch.Generator().manual_seed(seed)
    out = [(k, ops.draw_patchout(B, nrow, ncol, keep=k, generator=g)) for k in sorted({k for k in (1, 63, 64, 65, P - 1, P) if 1 <= k <= P})]
    k = max(P // 2, 1)
    out.append((k, ops.draw_patchout(1, nrow, ncol, keep=k, generator=g).expand(B, k).contiguous()))
    if P >= B:
        out.append((P // B, torch.randperm(P, generator=g)[:P // B * B].view(B, -1).sort(dim=1).values.to(I32)))
    return out


def operands(geo, C, D, exact, seed):
    T, F, p, s = geo
    g = torch.Generator().manual_seed(seed)
    P = ((T - p) // s + 1) * ((F - p) // s + 1)
    if exact:
        x = torch.randint(-2, 3, (B, C, T, F), generator=g).float()
        w = torch.randint(-1, 2, (D, C, p, p), generator=g).float().repeat(1, 3 // C, 1, 1)     # C = 1: three equal channels, exact mean
        cls, pos = torch.randint(-8, 9, (D,), generator=g) / 4.0, torch.randint(-8, 9, (P + 3, D), generator=g) / 4.0
    else:
        x, w = torch.randn(B, C, T, F, generator=g), torch.randn(D, 3, p, p, generator=g) * 0.05
        cls, pos = torch.randn(D, generator=g), torch.randn(P + 3, D, generator=g)
    pos_dev = pos.clone()
    pos_dev[P + 1:] = float("nan")          # rows beyond the sequence are never read
    return x, w, cls, pos, pos_dev, 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), P


def forward(ffi, geo, C, D, ops_dev, keep, want_patches=True, k=None, keep_ptr=True):
    T, F, p, s = geo
    x, w, cls, pos, gam, bet = ops_dev
    k = keep.shape[1] if k is None else k
    kcols, M = C * p * p, B * (k + 1)
    o = {"w_eff": Guarded((D, kcols), BF16, DEV), "patches": Guarded((B * max(k, 1), kcols), BF16, DEV), "tokens": Guarded((M, D), F32, DEV),
         "out": Guarded((M, D), F32, DEV), "mean": Guarded((M,), F32, DEV), "rstd": Guarded((M,), F32, DEV)}
    rc = ffi.lib().vipant_patch_embed_keep_ln_fwd(x.data_ptr(), w.data_ptr(), cls.data_ptr(), pos.data_ptr(), gam.data_ptr(), bet.data_ptr(),
                                                  keep.data_ptr() if keep_ptr else None, o["w_eff"].ptr(), o["patches"].ptr() if want_patches else None,
                                                  o["tokens"].ptr(), o["out"].ptr(), o["mean"].ptr(), o["rstd"].ptr(), B, C, T, F, D, 3, p, p, s, s,
                                                  k, int(C == 1), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, o


@pytest.mark.parametrize("geo,C,D", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "gauss"])
def test_forward(geo, C, D, exact):
    T, F, p, s = geo
    x, w, cls, pos, pos_dev, gam, bet, P = operands(geo, C, D, exact, seed=D + C)
    dev = tuple(nan_guarded(t) for t in (x, w, cls, pos_dev, gam, bet))
    cols = Fn.unfold(x.bfloat16().double(), (p, p), stride=s).transpose(1, 2)                    # [B, P, kcols], columns (c, ii, jj)
    im2col = torch.empty((B * P, C * p * p), dtype=BF16, device=DEV)
    ffi.call("vipant_im2col", dev[0].data_ptr(), im2col.data_ptr(), B, C, T, F, p, p, s, s, torch.cuda.current_stream().cuda_stream)
    for k, keep in keep_lists(ops, (T - p) // s + 1, (F - p) // s + 1, seed=P):
        rc, o = forward(ffi, geo, C, D, dev, keep.to(DEV))
        assert rc == 0, ffi.lib().vipant_last_error()
        [t.intact_around(name) for name, t in o.items()]
        W = o["w_eff"].v.cpu().double()
        idx = keep.long()
        A = torch.gather(cols, 1, idx.unsqueeze(2).expand(B, k, cols.shape[2]))
        ref = torch.cat([(cls.double() + pos[0].double()).expand(B, 1, D), A @ W.t() + pos.double()[1 + idx]], 1).reshape(-1, D)
        got = o["tokens"].v.cpu()
        if exact:
            assert bits(got, ref.float()), (k, float((got.double() - ref).abs().max()))
        else:
            bound = torch.cat([(cls.double().abs() + pos[0].double().abs()).expand(B, 1, D), A.abs() @ W.abs().t() + pos.double()[1 + idx].abs()], 1).reshape(-1, D)
            err = (got.double() - ref).abs()
            assert bool((err <= (C * p * p) * 2.0 ** -23 * bound).all()), (k, float(err.max()))
        rows = (torch.arange(B).unsqueeze(1) * P + idx).reshape(-1).to(DEV)
        assert bits(o["patches"].v, im2col[rows]), k
        _, y32, mean, rstd = ops.layernorm_fwd(o["tokens"].v, dev[4], dev[5], want_bf16=False, want_f32=True)
        assert bits(o["out"].v, y32) and bits(o["mean"].v, mean) and bits(o["rstd"].v, rstd), k
        rc, o2 = forward(ffi, geo, C, D, dev, keep.to(DEV), want_patches=False)
        assert rc == 0 and bits(o2["tokens"].v, o["tokens"].v) and bits(o2["out"].v, o["out"].v)
        o2["patches"].untouched("patches = NULL")
        if not exact:
            backward_checks(geo, C, D, dev, keep, o)


def backward_checks(geo, C, D, dev, keep, f):
    (T, F, p, s), k, kcols = geo, keep.shape[1], C * geo[2] * geo[2]
    P, M, keep_d = ((T - p) // s + 1) * ((F - p) // s + 1), B * (k + 1), keep.to(DEV)
    dout = nan_guarded(torch.randn(M, D, generator=torch.Generator().manual_seed(k)))
    ws = Workspace(ffi.query("vipant_patch_embed_keep_ln_bwd_workspace_bytes", B, k, D, kcols), DEV)
    runs = []
    for _ in range(2):
        o = {"inv": Guarded((B, P), I32, DEV, fill=-7), "dtokens": Guarded((M, D), F32, DEV), "dpatches": Guarded((B * k, D), BF16, DEV),
             "dw_eff": Guarded((D, kcols), F32, DEV), "dconv": Guarded((D, 3, p * p), F32, DEV), "dcls": Guarded((D,), F32, DEV),
             "dpos": Guarded((P + 3, D), F32, DEV), "dgamma": Guarded((D,), F32, DEV), "dbeta": Guarded((D,), F32, DEV)}
        ffi.call("vipant_patch_embed_keep_ln_bwd", dout.data_ptr(), 0, f["tokens"].ptr(), f["mean"].ptr(), f["rstd"].ptr(), dev[4].data_ptr(),
                 f["patches"].ptr(), keep_d.data_ptr(), o["inv"].ptr(), o["dtokens"].ptr(), o["dpatches"].ptr(), o["dw_eff"].ptr(),
                 o["dconv"].ptr(), o["dcls"].ptr(), o["dpos"].ptr(), o["dgamma"].ptr(), o["dbeta"].ptr(), B, k, P, D, 3, p * p, int(C == 1),
                 ws.ptr(), ws.n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ws.intact_around("workspace")
        [t.intact_around(name) for name, t in o.items()]
        runs.append(o)
    o = runs[0]
    assert all(bits(runs[1][n].v, o[n].v) for n in o), "two runs differ"
    dt = o["dtokens"].v.cpu().view(B, k + 1, D)
    assert bits(o["dpatches"].v.cpu(), dt[:, 1:].reshape(B * k, D).to(BF16)), k
    ref, mag = torch.zeros(P + 1, D, dtype=F64), torch.zeros(P + 1, D, dtype=F64)
    rows = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + keep.long()], 1).reshape(-1)
    ref.index_add_(0, rows, dt.reshape(-1, D).double())
    mag.index_add_(0, rows, dt.reshape(-1, D).double().abs())
    dpos = o["dpos"].v.cpu()
    assert bool(((dpos[:P + 1].double() - ref).abs() <= B * 2.0 ** -24 * mag).all()), k          # (unkept rows: bound 0, exactly 0)
    assert bits(o["dcls"].v.cpu(), dpos[0]) and bool((dpos[P + 1:] == FILL).all()), k
    want = ops.gemm_tn(o["dpatches"].v, f["patches"].v, torch.empty((D, kcols), dtype=F32, device=DEV))
    assert bits(o["dw_eff"].v, want), k


def test_refusals_write_nothing():
    geo, C, D = GEOS[0], 1, 192
    x, w, cls, pos, pos_dev, gam, bet, P = operands(geo, C, D, True, seed=1)
    dev = tuple(nan_guarded(t) for t in (x, w, cls, pos_dev, gam, bet))
    keep = ops.draw_patchout(B, 7, 4, keep=P).to(DEV)
    for k, ptr in ((0, True), (P + 1, True), (P, False)):
        rc, o = forward(ffi, geo, C, D, dev, keep, k=k, keep_ptr=ptr)
        assert rc == -1, (k, ptr, rc)
        [t.untouched(f"{name} (k={k}, keep {'given' if ptr else 'NULL'})") for name, t in o.items()]
