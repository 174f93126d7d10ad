"""vipant_layernorm_fwd / _bwd at widths 64 H that are no multiple of 256 (csrc/layernorm_widths.hip) against fp64 layer_norm and its
autograd.  D: 192 (no full 64-lane step), 320 / 384 / 448 (lane groups), 960 (widest ragged row); M: 1, 5 (partial last workgroup), 37
(partial rounds of the backward's ring).  Bounds: tests/test_kernels_gpu.py::test_layernorm, test_layernorm_fp16_stream."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from guards import FILL, Guarded, Workspace, poisoned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
EBADSHAPE = -1
st = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
dev = lambda t: t.to(DEV).contiguous()                    # noqa: E731
SHAPES = [(D, M) for D in (192, 320, 384, 448, 960) for M in (1, 5, 37)]


@pytest.fixture(scope="module")
def ffi():
    from vipant_amd import _ffi
    _ffi.call("vipant_device_check")
    return _ffi


def assert_close(got, ref, rtol, atol, what):
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - ref).abs()
    print(f"{what}: worst error / bound {float((err / (atol + rtol * ref.abs())).max()):.3f}")
    assert bool((err <= atol + rtol * ref.abs()).all()), f"{what}: max error {float(err.max()):.4e} at scale {float(ref.abs().max()):.3e}"


@functools.lru_cache(maxsize=None)
def case(D, M):
    g = torch.Generator().manual_seed(1000 * D + M)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(M, D) * 2 + 0.3, x16=(r(M, D) * 3).to(F16), add=r(M, D).to(BF16), gamma=r(D) * 0.1 + 1.0, beta=r(D) * 0.1,
                dy=r(M, D).to(BF16), dy32=r(M, D), dres=r(M, D), dg0=r(D), db0=r(D))


def reference(x, gamma, beta, dy=None):
    """fp64 (y, mean, rstd[, dx, dgamma, dbeta])."""
    x, gamma, beta = (t.double().clone().requires_grad_() for t in (x, gamma, beta))
    y = F.layer_norm(x, x.shape[-1:], gamma, beta, 1e-5)
    mean, rstd = x.detach().mean(-1), (x.detach().var(-1, unbiased=False) + 1e-5).rsqrt()
    if dy is None:
        return y.detach(), mean, rstd
    y.backward(dy.double())
    return y.detach(), mean, rstd, x.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("form", ["plain", "add", "f16", "strided"])
@pytest.mark.parametrize("D,M", SHAPES)
def test_forward(ffi, D, M, form):
    c = case(D, M)
    f16, add = form == "f16", form in ("add", "f16")
    ldx = 3 * D if form == "strided" else D
    x = poisoned(dev(c["x16"] if f16 else c["x"]), ldx, 0, 1)       # NaN in the rows' padding and in a row behind the last
    o = dict(y=Guarded((M, D), BF16, DEV), y32=Guarded((M, D), F32, DEV), mean=Guarded((M,), F32, DEV), rstd=Guarded((M,), F32, DEV),
             sum=Guarded((M, D), F16 if f16 else F32, DEV))
    gamma_d, beta_d, add_d = dev(c["gamma"]), dev(c["beta"]), dev(c["add"])
    rc = ffi.lib().vipant_layernorm_fwd(x.data_ptr(), ldx, gamma_d.data_ptr(), beta_d.data_ptr(), o["y"].ptr(), o["y32"].ptr(),
                                        o["mean"].ptr(), o["rstd"].ptr(), M, D, add_d.data_ptr() if add else None,
                                        o["sum"].ptr() if add else None, None, None,
                                        (ffi.STREAM_IN_F16 | ffi.STREAM_OUT_F16) if f16 else 0, st())
    torch.cuda.synchronize()
    assert rc == 0, ffi.lib().vipant_last_error()
    for k, v in o.items():
        v.intact_around(f"layernorm_fwd {form}: {k}")
    s64 = (c["x16"] if f16 else c["x"]).double() + (c["add"].double() if add else 0)
    y, mean, rstd = reference(s64, c["gamma"], c["beta"])
    if add:
        assert torch.equal(o["sum"].v.cpu(), s64.float().to(F16) if f16 else s64.float()), "the stored stream is the rounding of the exact sum"
    else:
        o["sum"].untouched("layernorm_fwd without add: sum_out")
    assert_close(o["y"].v, y, 1e-2, 1e-2, "y bf16")
    assert_close(o["mean"].v, mean, 1e-5, 1e-5, "mean")
    if not f16:     # (test_layernorm_fp16_stream bounds the bf16 output and the mean)
        assert_close(o["y32"].v, y, 1e-5, 1e-5, "y fp32")
        assert_close(o["rstd"].v, rstd, 1e-5, 1e-5, "rstd")


@pytest.mark.parametrize("form", ["bf16dy", "f32dy", "bf16dres", "accumulate"])
@pytest.mark.parametrize("D,M", SHAPES)
def test_backward(ffi, D, M, form):
    c = case(D, M)
    dy = c["dy32"] if form == "f32dy" else c["dy"]
    res = form in ("bf16dy", "bf16dres")
    dres = c["dres"].to(BF16) if form == "bf16dres" else c["dres"]
    _, mean, rstd, dx64, dg64, db64 = reference(c["x"], c["gamma"], c["beta"], dy)
    if res:
        dx64 = dx64 + dres.double()
    ld = 3 * D if form == "bf16dy" else D                 # strided x, dres and dx with NaN / sentinels in the padding
    x = poisoned(dev(c["x"]), ld, 0, 1)
    dres_d = poisoned(dev(dres), D if form == "bf16dres" else ld, 0, 1) if res else None
    acc = form == "accumulate"
    nbytes = ffi.query("vipant_layernorm_bwd_workspace_bytes", M, D)
    flags = (ffi.LN_DY_F32 if form == "f32dy" else 0) | (ffi.LN_DRES_BF16 if form == "bf16dres" else 0)
    dy_d, mean_d, rstd_d, gamma_d = dev(dy), dev(mean.float()), dev(rstd.float()), dev(c["gamma"])
    runs = []
    for _ in range(2):                                    # twice from a dirty exact-size workspace: the same bits
        ws = Workspace(nbytes, DEV)
        o = dict(dx=Guarded((M, ld), F32, DEV), dxb=Guarded((M, D), BF16, DEV), dcs=Guarded((D,), F32, DEV),
                 dg=Guarded((D,), F32, DEV, init=dev(c["dg0"]) if acc else None), db=Guarded((D,), F32, DEV, init=dev(c["db0"]) if acc else None))
        rc = ffi.lib().vipant_layernorm_bwd(dy_d.data_ptr(), flags, x.data_ptr(), ld, mean_d.data_ptr(), rstd_d.data_ptr(), gamma_d.data_ptr(),
                                            dres_d.data_ptr() if res else None, None if form == "bf16dres" else o["dx"].ptr(), ld,
                                            o["dxb"].ptr() if res else None, o["dg"].ptr(), o["db"].ptr(),
                                            o["dcs"].ptr() if form == "bf16dy" else None, int(acc), M, D, ws.ptr(), nbytes, None, None, st())
        torch.cuda.synchronize()
        assert rc == 0, ffi.lib().vipant_last_error()
        ws.intact_around("layernorm_bwd")
        for k, v in o.items():
            v.intact_around(f"layernorm_bwd {form}: {k}")
        assert bool((o["dx"].v[:, D:] == FILL).all()), "the padding of dx rows was written"
        runs.append(o)
    for k in o:
        assert torch.equal(runs[0][k].parent, runs[1][k].parent), f"{k}: two runs differ"
    tail = 1e-3 * math.sqrt(M)
    if form != "bf16dres":
        assert_close(o["dx"].v[:, :D], dx64, 1e-4, 1e-4, "dx")
    if res:
        assert_close(o["dxb"].v, dx64, 1e-2, 1e-2, "dx bf16")
    if form == "bf16dy":
        assert_close(o["dcs"].v, dx64.sum(0), 1e-4, tail, "dx colsum")
    assert_close(o["dg"].v, dg64 + (c["dg0"].double() if acc else 0), 1e-4, tail, "dgamma")
    assert_close(o["db"].v, db64 + (c["db0"].double() if acc else 0), 1e-4, tail, "dbeta")


@pytest.mark.parametrize("D,q8", [(64, False), (128, False), (200, False), (1088, False), (384, True)])
def test_refusals_write_nothing(ffi, D, q8):
    """No kernel of that width; no e4m3 output (q / qscale) at a width the lane-group kernels serve."""
    M = 5
    x, vec, stat = torch.ones(M, D, device=DEV), torch.ones(D, device=DEV), torch.ones(M, device=DEV)
    dyb = torch.ones(M, D, dtype=BF16, device=DEV)
    q, qs = Guarded((M, D), torch.uint8, DEV), Guarded((4096,), torch.uint8, DEV)
    o = dict(y=Guarded((M, D), BF16, DEV), y32=Guarded((M, D), F32, DEV), mean=Guarded((M,), F32, DEV), rstd=Guarded((M,), F32, DEV), q=q, qs=qs,
             dx=Guarded((M, D), F32, DEV), dxb=Guarded((M, D), BF16, DEV), dg=Guarded((D,), F32, DEV), db=Guarded((D,), F32, DEV))
    L = ffi.lib()
    rc = L.vipant_layernorm_fwd(x.data_ptr(), D, vec.data_ptr(), vec.data_ptr(), o["y"].ptr(), o["y32"].ptr(), o["mean"].ptr(), o["rstd"].ptr(),
                                M, D, None, None, q.ptr() if q8 else None, qs.ptr() if q8 else None, 0, st())
    assert rc == EBADSHAPE and b"layernorm_fwd" in L.vipant_last_error(), rc
    ws = Workspace(256 * 3 * D * 4, DEV)
    rc = L.vipant_layernorm_bwd(dyb.data_ptr(), 0, x.data_ptr(), D, stat.data_ptr(), stat.data_ptr(), vec.data_ptr(), None, o["dx"].ptr(), D,
                                o["dxb"].ptr(), o["dg"].ptr(), o["db"].ptr(), None, 0, M, D, ws.ptr(), ws.n, q.ptr() if q8 else None,
                                qs.ptr() if q8 else None, st())
    torch.cuda.synchronize()
    assert rc == EBADSHAPE and b"layernorm_bwd" in L.vipant_last_error(), rc
    ws.untouched("layernorm_bwd refused")
    for k, v in o.items():
        v.untouched(f"refused at D={D}: {k}")
