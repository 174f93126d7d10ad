"""vipant_layernorm_fwd / _bwd at the widths of the production towers, D = 256, 512, 768, 1024 (csrc/layernorm.hip), through the C ABI:
every compiled instance, the optional outputs, the in-place aliases of the block backward and the row strides of the token-boundary
operators, against an fp64 reference taken on the device.  The ragged widths have tests/test_ln_widths_gpu.py; this is the same for
the main ones.

Rows.  M = 1, 5, 37 for every form, M = 4100 for one forward and two backward forms per width.  The forward runs one row per wave,
four waves per workgroup: 1, 5, 37 and 4100 all leave a partial last workgroup.  The backward's waves walk rows wave, wave + nwaves,
... through a two-row ring, ln_blocks(M) = min(ceil(M / 16), 256) workgroups: M = 5 is one workgroup whose wave 0 takes rows 0 and 4
(the prefetch) and whose other waves take one; M = 37 is three workgroups whose waves take 3 or 4 rows (the ring wraps; odd and even
counts); M = 4100 reaches the grid cap (1024 waves, 4 or 5 rows each) and a finalize that sums 256 partial rows, 16 per lane group.

Inputs.  One matrix per (D, M) whose row r belongs to family r % 6: N(0.3, 2); +-100 + N(0, 1); N(0, 1) 2^k with k cycling over
-8 .. 8; the constant 3.7; zero; one element 1e3 at column 7 r % D (|xhat| = sqrt(D - 1) there).  The fp16 streams take its fp16
rounding, and the reference sees that.  x, an fp32 dres and dx_f32 live in parents of row length 3 D whose other elements (and one row
behind the last) are NaN (inputs) or the sentinel (outputs); every output has guard zones; every workspace is dirty and exactly as
large as the library asks for; every backward case runs twice and must give the same bits.

Bounds.  Those of tests/test_kernels_gpu.py::test_layernorm and tests/test_ln_widths_gpu.py -- y fp32 1e-5 / 1e-5, y bf16 1e-2 /
1e-2, mean 1e-5 / 1e-5, rstd 1e-5 relative; dx fp32 1e-4 / 1e-4, dx bf16 1e-2 / 1e-2, the column sums 1e-4 relative + 1e-3 sqrt(M)
-- and in the forward one derived term for a row whose mean dwarfs its spread: an fp32 sum over the row of depth D / 64 + 6 (D / 256
four-element steps of a lane, four elements each, six shuffle stages: rounded up) leaves the mean off by at most depth 2^-24 |mean|;
carried into xhat that is T = depth 2^-24 |mean| rstd |gamma|, added to both y bounds; the mean gets depth 2^-24 |mean|, rstd
depth 2^-23 |mean| rstd^2 (to first order in the variance error of a shifted mean).  The terms come from the arithmetic, not from
what the kernel gives: a two-pass fp32 kernel uses about a tenth of T on the +-100 rows, a one-pass variance misses it 20 - 40 fold.
No family needed a further term in the backward: the reference there is the entry point's own statement in fp64 on the fp32 roundings
of the fp64 statistics (as tests/test_ln_pair_gpu.py has it), so the cancellation in x - mean is the same on both sides.
The stored stream is checked as the project's tests always have (test_layernorm_fp16_stream): the fp32 sum, which the fp64 sum
rounds to, and for an fp16 stream that sum's fp16 rounding.

Coverage: every instance the launchers can select, at each of the four widths (and each of M = 1, 5, 37).

  forward  stream in / out   plain kernel                                          e4m3 kernel (q, qscale)
           fp32 / fp32       test_forward_outputs[plain | y32only | yonly],        test_forward_q8[f32f32]
                             test_forward_add[f32f32], test_forward_add_without_sum
           fp32 / fp16       test_forward_add[f32f16]                              test_forward_q8[f32f16]
           fp16 / fp32       test_forward_add[f16f32]                              test_forward_q8[f16f32]
           fp16 / fp16       test_forward_add[f16f16] (also M = 4100)              test_forward_q8[f16f16]

  backward dy / dres         x fp32 and x fp16 (LN_X_F16), plain kernel            e4m3 kernel (q, qscale)
           bf16 / fp32, none test_backward[separate | inplace32 (also M = 4100) |  test_backward_q8[inplace32]
                             strides | accumulate]
           bf16 / bf16       test_backward[inplace16] (also M = 4100)              test_backward_q8[inplace16]
           fp32 / none       test_backward[f32dy]                                  test_backward_f32dy_q8 (D = 256 only: compiled
                                                                                   at every width, but no caller passes q with an
                                                                                   fp32 dy)
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from guards import FILL, Guarded, Workspace, poisoned
from mx_emul import check_block_uniform_form, mx_scales

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16, U8 = torch.float32, torch.float16, torch.bfloat16, torch.uint8
EBADSHAPE, EALIGN, ENOWORKSPACE = -1, -3, -5
WIDTHS = (256, 512, 768, 1024)
SMALL = [(D, M) for D in WIDTHS for M in (1, 5, 37)]
BIG_M = 4100
ZERO_BLOCK, LOUD_BLOCK = 1, 3         # e4m3 cases: gamma = beta = 0 in columns [32, 64), |gamma| 16-fold in columns [96, 128)
st = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
G = lambda shape, dtype, init=None: Guarded(shape, dtype, DEV, init=init)      # noqa: E731


@pytest.fixture(scope="module")
def ffi():
    from vipant_amd import _ffi
    _ffi.call("vipant_device_check")
    return _ffi


@pytest.fixture(scope="module")
def ops():
    from vipant_amd import ops as O
    return O


def depth(D):
    return D // 64 + 6


def check(tag, got, ref, rtol, atol, extra=None):
    """|got - ref| <= atol + rtol |ref| (+ extra), and the worst error / bound is printed."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{tag}: non-finite output"
    bound = atol + rtol * ref.abs()
    if extra is not None:
        bound = bound + extra
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    print(f"ln parity: {tag}: worst error / bound {float(ratio.max()):.3f}")
    assert bool((err <= bound).all()), f"{tag}: error / bound {float(ratio.max()):.3f}, max error {float(err.max()):.4e}"


def family_rows(M, D, g):
    """[M, D] fp32 (CPU): row r is of family r % 6 (module docstring)."""
    row = torch.arange(M)
    fam, occ = (row % 6)[:, None], row // 6
    n = torch.randn(M, D, generator=g)
    x = n * 2 + 0.3
    x = torch.where(fam == 1, torch.where(occ % 2 == 0, 100.0, -100.0)[:, None] + n, x)
    x = torch.where(fam == 2, n * torch.exp2((occ % 17 - 8).float())[:, None], x)
    x = torch.where(fam == 3, torch.full_like(x, 3.7), x)
    x = torch.where(fam == 4, torch.zeros_like(x), x)
    spike = torch.zeros(M, D)
    spike[row, (7 * row) % D] = 1e3
    return torch.where(fam == 5, spike, x)


@functools.lru_cache(maxsize=None)
def case(D, M, device=DEV):
    g = torch.Generator().manual_seed(1000 * D + M)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    x = family_rows(M, D, g)
    c = dict(x=x, x16=x.to(F16), add=r(M, D).to(BF16), gamma=r(D) * 0.1 + 1.0, beta=r(D) * 0.1, dy=r(M, D).to(BF16), dy32=r(M, D),
             dres=r(M, D), dg0=r(D), db0=r(D), dcs0=r(D))
    c["dres16"] = r(M, D).to(BF16)
    gq, bq = c["gamma"].clone(), c["beta"].clone()
    gq[32 * ZERO_BLOCK:32 * ZERO_BLOCK + 32] = 0
    bq[32 * ZERO_BLOCK:32 * ZERO_BLOCK + 32] = 0
    gq[32 * LOUD_BLOCK:32 * LOUD_BLOCK + 32] *= 16
    c["gamma_q"], c["beta_q"] = gq, bq
    c = {k: v.to(device).contiguous() for k, v in c.items()}
    c["fam"] = (torch.arange(M) % 6).to(device)
    return c


@functools.lru_cache(maxsize=None)
def fwd_ref(D, M, in16, add, q, device=DEV):
    """fp64 layer_norm of the exact input (x + add in fp64), its fp64 mean and rstd, and the derived term T (module docstring)."""
    c = case(D, M, device)
    s = c["x16" if in16 else "x"].double() + (c["add"].double() if add else 0)
    gamma, beta = (c["gamma_q"], c["beta_q"]) if q else (c["gamma"], c["beta"])
    mean, rstd = s.mean(-1), (s.var(-1, unbiased=False) + 1e-5).rsqrt()
    y = F.layer_norm(s, (D,), gamma.double(), beta.double(), 1e-5)
    t_stat = depth(D) * 2.0 ** -24 * mean.abs()
    return dict(s=s, y=y, mean=mean, rstd=rstd, T=(t_stat * rstd)[:, None] * gamma.double().abs()[None, :], t_mean=t_stat,
                t_rstd=2 * t_stat * rstd * rstd)


def run_fwd(ffi, D, M, *, in16=False, out16=False, add=False, want_sum=True, y=True, y32=True, q=False, gq=False, x=None, ldx=None):
    """One call; returns the Guarded outputs that were passed.  The others must keep the sentinel.  gq: the gamma / beta of the e4m3 cases."""
    c = case(D, M)
    if x is None:
        ldx = 3 * D
        x = poisoned(c["x16" if in16 else "x"], ldx, 0, 1)            # NaN in the rows' padding and in a row behind the last
    o = dict(y=G((M, D), BF16), y32=G((M, D), F32), mean=G((M,), F32), rstd=G((M,), F32), sum=G((M, D), F16 if out16 else F32),
             q=G((M, D), U8), qs=G((ffi.query("vipant_mx_scale_bytes", M, D),), U8))
    gamma, beta = (c["gamma_q"], c["beta_q"]) if q or gq else (c["gamma"], c["beta"])
    passed = dict(y=y, y32=y32, mean=True, rstd=True, sum=add and want_sum, q=q, qs=q)
    p = {k: (o[k].ptr() if passed[k] else None) for k in o}
    rc = ffi.lib().vipant_layernorm_fwd(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), p["y"], p["y32"], p["mean"], p["rstd"], M, D,
                                        c["add"].data_ptr() if add else None, p["sum"], p["q"], p["qs"],
                                        (ffi.STREAM_IN_F16 if in16 else 0) | (ffi.STREAM_OUT_F16 if out16 else 0), st())
    torch.cuda.synchronize()
    assert rc == 0, ffi.lib().vipant_last_error()
    for k, v in o.items():
        if passed[k]:
            v.intact_around(f"layernorm_fwd: {k}")
        else:
            v.untouched(f"layernorm_fwd: {k} was not passed")
    return {k: v for k, v in o.items() if passed[k]}


def check_fwd(tag, o, ref, D, plain_rows=None):
    """The outputs that were written against the fp64 reference; plain_rows: the case has no add, so its all-zero rows are exact."""
    if "y32" in o:
        check(f"{tag} y_f32", o["y32"].v, ref["y"], 1e-5, 1e-5, ref["T"])
    if "y" in o:
        check(f"{tag} y", o["y"].v, ref["y"], 1e-2, 1e-2, ref["T"])
    check(f"{tag} mean", o["mean"].v, ref["mean"], 1e-5, 1e-5, ref["t_mean"])
    check(f"{tag} rstd", o["rstd"].v, ref["rstd"], 1e-5, 0.0, ref["t_rstd"])
    if plain_rows is not None:
        zero = plain_rows["fam"] == 4
        if bool(zero.any()):
            beta = plain_rows["beta"]
            assert bool((o["mean"].v[zero] == 0).all()), f"{tag}: the mean of an all-zero row"
            if "y32" in o:
                assert torch.equal(o["y32"].v[zero], beta.expand(int(zero.sum()), D)), f"{tag}: y_f32 of an all-zero row is beta"
            if "y" in o:
                assert torch.equal(o["y"].v[zero], beta.to(BF16).expand(int(zero.sum()), D)), f"{tag}: y of an all-zero row is beta"


@pytest.mark.parametrize("form", ["plain", "y32only", "yonly"])
@pytest.mark.parametrize("D,M", SMALL)
def test_forward_outputs(ffi, D, M, form):
    """fp32 rows at ldx = 3 D, no add; y = NULL is the ln_post / patch call, y_f32 = NULL the block's; the absent buffer keeps its sentinel."""
    o = run_fwd(ffi, D, M, y=form != "y32only", y32=form != "yonly")
    check_fwd(f"fwd D={D} M={M} {form}", o, fwd_ref(D, M, False, False, False), D, plain_rows=case(D, M))


PAIRS = {"f32f32": (False, False), "f32f16": (False, True), "f16f32": (True, False), "f16f16": (True, True)}


@pytest.mark.parametrize("D,M,pair", [(D, M, p) for D, M in SMALL for p in PAIRS] + [(D, BIG_M, "f16f16") for D in WIDTHS])
def test_forward_add(ffi, D, M, pair):
    """The residual add in front of the norm, for every stream type pair: the stored stream is the rounding of the exact sum, and the
    norm is taken on the UNROUNDED sum -- y, mean and rstd have the bits of the fp32-out run, whose stored sum is that unrounded sum,
    and of a plain call on it."""
    in16, out16 = PAIRS[pair]
    ref = fwd_ref(D, M, in16, True, False)
    o = run_fwd(ffi, D, M, in16=in16, out16=out16, add=True)
    check_fwd(f"fwd D={D} M={M} add_{pair}", o, ref, D)
    s32 = ref["s"].float()
    assert torch.equal(o["sum"].v, s32.to(F16) if out16 else s32), "the stored stream is the rounding of the exact sum"
    o32 = run_fwd(ffi, D, M, in16=in16, out16=False, add=True) if out16 else o
    assert torch.equal(o32["sum"].v, s32)
    back = run_fwd(ffi, D, M, x=poisoned(o32["sum"].v, 3 * D, 0, 1), ldx=3 * D)          # a plain fp32 call on the stored sum
    for k in ("y", "y32", "mean", "rstd"):
        assert torch.equal(o[k].v, o32[k].v), f"{k}: the norm of the {pair} run is not the one of the unrounded sum"
        assert torch.equal(o[k].v, back[k].v), f"{k}: x + add fused differs from a plain call on the sum"


@pytest.mark.parametrize("D,M", SMALL)
def test_forward_add_without_sum(ffi, D, M):
    """add with sum_out = NULL: nothing but y, mean and rstd is written (run_fwd finds every other buffer untouched)."""
    o = run_fwd(ffi, D, M, add=True, want_sum=False, y32=False)
    check_fwd(f"fwd D={D} M={M} add_nosum", o, fwd_ref(D, M, False, True, False), D)


@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("D,M", SMALL)
def test_forward_q8(ffi, ops, D, M, pair):
    """The e4m3 output beside y: static scales, one per 32-column block and the same for every row, from sqrt(D) |gamma| + |beta|.  The
    spike rows (M = 37) reach |xhat| = sqrt(D - 1): nothing may saturate there.  Everything else has the bits of the call without q."""
    in16, out16 = PAIRS[pair]
    c = case(D, M)
    o = run_fwd(ffi, D, M, in16=in16, out16=out16, add=True, q=True)
    check_fwd(f"fwd D={D} M={M} q8_{pair}", o, fwd_ref(D, M, in16, True, True), D)
    base = run_fwd(ffi, D, M, in16=in16, out16=out16, add=True, gq=True)
    for k, v in base.items():
        assert torch.equal(o[k].parent, v.parent), f"{k}: the call with q differs from the call without"
    gamma, beta = c["gamma_q"], c["beta_q"]
    # the block-uniform form of y: never below what a block's largest element needs, bytes exactly y / 2^e in e4m3
    sc = mx_scales(ops, o["qs"].v, M, D).int()
    check_block_uniform_form(ops, (o["q"].v, o["qs"].v), o["y"].v, slack=8)
    # the scales: identical for every row, between what the static bound needs and one binade above
    assert bool((sc == sc[0:1]).all()), "the scales differ between rows"
    bound = (gamma.double().abs() * math.sqrt(D) + beta.double().abs()).view(D // 32, 32).amax(dim=1)
    live = bound > 0
    e_need = torch.ceil(torch.log2(bound[live] / 448)).int() + 127
    assert bool((sc[0][live] >= e_need).all()) and bool((sc[0][live] <= e_need + 1).all()), (sc[0][live] - e_need)
    scale = torch.exp2(sc.double() - 127)[:, :, None].expand(M, D // 32, 32).reshape(M, D)
    assert float((o["y"].v.double().abs() / scale).max()) <= 448, "an element saturates under the static scale"
    assert torch.equal(o["q"].v, (o["y"].v.double() / scale).float().to(torch.float8_e4m3fn).view(U8)), "bytes are not y / 2^e in e4m3"
    assert bool((~live).sum() == 1) and bool((o["q"].v[:, 32 * ZERO_BLOCK:32 * ZERO_BLOCK + 32] == 0).all()), "the gamma = beta = 0 block"


# ------------------------------------------------------------------------------------------------------------------------ backward
#        flags               dres         ldx lddx  dx     dxb    dcs   (ld in units of D)
BWD = {
    "separate":  ("",        "f32",       3,  3,    True,  True,  True),       # every output, every stride
    "inplace32": ("",        "alias32",   1,  1,    True,  True,  True),       # dres == dx_f32: the block backward's fp32 stream gradient
    "inplace16": ("dres16",  "alias16",   1,  1,    False, True,  True),       # dres == dx_bf16, dx_f32 = NULL: its bf16 stream gradient
    "f32dy":     ("dy32",    None,        3,  3,    True,  False, False),      # the patch / ln_post call
    "strides":   ("",        None,        3,  1,    True,  True,  True),       # rows of a [b, S, D] tensor in, contiguous rows out
    "accumulate": ("",       None,        3,  1,    True,  False, True),       # dgamma, dbeta and dx_colsum receive +=
}


@functools.lru_cache(maxsize=None)
def bwd_ref(D, M, x16, dy32, dres, device=DEV):
    """The entry point's own statement in fp64, on the fp32 roundings of the fp64 statistics."""
    c = case(D, M, device)
    x = c["x16" if x16 else "x"].double()
    mean32, rstd32 = x.mean(-1).float(), (x.var(-1, unbiased=False) + 1e-5).rsqrt().float()
    dy, gamma = c["dy32" if dy32 else "dy"].double(), c["gamma"].double()
    rs = rstd32.double()[:, None]
    xhat = (x - mean32.double()[:, None]) * rs
    g = dy * gamma
    dx = rs * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + c[dres].double()
    return dict(mean32=mean32.contiguous(), rstd32=rstd32.contiguous(), dx=dx, dg=(dy * xhat).sum(0), db=dy.sum(0), dcs=dx.sum(0))


def run_bwd(ffi, D, M, form, x16, q=False):
    """One call from a fresh dirty workspace and fresh guarded outputs."""
    mode, dres_kind, ldx, lddx, want_dx, want_dxb, want_dcs = BWD[form]
    ldx, lddx = ldx * D, lddx * D
    c = case(D, M)
    acc = form == "accumulate"
    ref = bwd_ref(D, M, x16, mode == "dy32", {None: None, "f32": "dres", "alias32": "dres", "alias16": "dres16"}[dres_kind])
    x = poisoned(c["x16" if x16 else "x"], ldx, 0, 1)
    o = dict(dx=G((M, lddx), F32), dxb=G((M, D), BF16), dcs=G((D,), F32, c["dcs0"] if acc else None), dg=G((D,), F32, c["dg0"] if acc else None),
             db=G((D,), F32, c["db0"] if acc else None), q=G((M, D), U8), qs=G((ffi.query("vipant_mx_scale_bytes", M, D),), U8))
    dres = None
    if dres_kind == "f32":
        dres = poisoned(c["dres"], lddx, 0, 1)
        dres_ptr = dres.data_ptr()
    elif dres_kind == "alias32":
        o["dx"].v.copy_(c["dres"])
        dres_ptr = o["dx"].ptr()
    elif dres_kind == "alias16":
        o["dxb"].v.copy_(c["dres16"])
        dres_ptr = o["dxb"].ptr()
    else:
        dres_ptr = None
    nbytes = ffi.query("vipant_layernorm_bwd_workspace_bytes", M, D)
    ws = Workspace(nbytes, DEV)
    flags = (ffi.LN_DY_F32 if mode == "dy32" else 0) | (ffi.LN_DRES_BF16 if mode == "dres16" else 0) | (ffi.LN_X_F16 if x16 else 0)
    passed = dict(dx=want_dx, dxb=want_dxb, dcs=want_dcs, dg=True, db=True, q=q, qs=q)
    p = {k: (o[k].ptr() if passed[k] else None) for k in o}
    rc = ffi.lib().vipant_layernorm_bwd(c["dy32" if mode == "dy32" else "dy"].data_ptr(), flags, x.data_ptr(), ldx, ref["mean32"].data_ptr(),
                                        ref["rstd32"].data_ptr(), c["gamma"].data_ptr(), dres_ptr, p["dx"], lddx, p["dxb"], p["dg"], p["db"],
                                        p["dcs"], int(acc), M, D, ws.ptr(), nbytes, p["q"], p["qs"], st())
    torch.cuda.synchronize()
    assert rc == 0, ffi.lib().vipant_last_error()
    ws.intact_around(f"layernorm_bwd {form}")
    for k, v in o.items():
        if passed[k]:
            v.intact_around(f"layernorm_bwd {form}: {k}")
        else:
            v.untouched(f"layernorm_bwd {form}: {k} was not passed")
    if want_dx:
        assert bool((o["dx"].v[:, D:] == FILL).all()), "the padding of the dx rows was written"
    return {k: v for k, v in o.items() if passed[k]}, ref


def run_bwd_twice(ffi, D, M, form, x16, q=False):
    """The values of the first run against the reference, then a second run from another dirty workspace: the same bits (no atomics)."""
    a, ref = run_bwd(ffi, D, M, form, x16, q)
    check_bwd(f"bwd D={D} M={M} {'q8_' if q else ''}{form} {'x16' if x16 else 'x32'}", a, ref, D, M, form)
    b, _ = run_bwd(ffi, D, M, form, x16, q)
    for k in a:
        assert torch.equal(a[k].parent, b[k].parent), f"{form}: {k} differs between two runs"
    return a, ref


def check_bwd(tag, o, ref, D, M, form):
    _, _, _, _, want_dx, want_dxb, want_dcs = BWD[form]
    c = case(D, M)
    acc = form == "accumulate"
    tail = 1e-3 * math.sqrt(M)
    if want_dx:
        check(f"{tag} dx", o["dx"].v[:, :D], ref["dx"], 1e-4, 1e-4)
    if want_dxb:
        check(f"{tag} dx_bf16", o["dxb"].v, ref["dx"], 1e-2, 1e-2)
    if want_dcs:
        check(f"{tag} dx_colsum", o["dcs"].v, ref["dcs"] + (c["dcs0"].double() if acc else 0), 1e-4, tail)
    check(f"{tag} dgamma", o["dg"].v, ref["dg"] + (c["dg0"].double() if acc else 0), 1e-4, tail)
    check(f"{tag} dbeta", o["db"].v, ref["db"] + (c["db0"].double() if acc else 0), 1e-4, tail)


@pytest.mark.parametrize("x16", [False, True], ids=["x32", "x16"])
@pytest.mark.parametrize("D,M,form", [(D, M, f) for D, M in SMALL for f in BWD] + [(D, BIG_M, f) for D in WIDTHS for f in ("inplace32", "inplace16")])
def test_backward(ffi, D, M, form, x16):
    """Every form of BWD against the fp64 statement of the entry point, twice from dirty workspaces with the same bits.  No family of
    rows needed a term beyond the project's bounds (module docstring); the worst error / bound of each quantity is printed."""
    run_bwd_twice(ffi, D, M, form, x16)


def quantised_alone(ffi, ops, dxb, M, D):
    """(bytes, scale bytes [M, D / 32]) that vipant_quant_e4m3_mx makes of the bf16 matrix."""
    q, qs = G((M, D), U8), G((ffi.query("vipant_mx_scale_bytes", M, D),), U8)
    dxb = dxb.contiguous()
    ffi.call("vipant_quant_e4m3_mx", dxb.data_ptr(), D, q.ptr(), D, qs.ptr(), M, D, st())
    torch.cuda.synchronize()
    q.intact_around("quant_e4m3_mx: q")
    qs.intact_around("quant_e4m3_mx: scales")
    return q.v, mx_scales(ops, qs.v, M, D)


@pytest.mark.parametrize("x16", [False, True], ids=["x32", "x16"])
@pytest.mark.parametrize("form", ["inplace32", "inplace16"])
@pytest.mark.parametrize("D,M", SMALL)
def test_backward_q8(ffi, ops, D, M, form, x16):
    """q / qscale beside the stream gradient: every other output has the bits of the call without them, and the bytes and block scales
    are those of vipant_quant_e4m3_mx on the bf16 gradient the call produced."""
    o, _ = run_bwd_twice(ffi, D, M, form, x16, q=True)
    base, _ = run_bwd(ffi, D, M, form, x16, q=False)
    for k in base:
        assert torch.equal(o[k].parent, base[k].parent), f"{k}: the call with q differs from the call without"
    q_ref, s_ref = quantised_alone(ffi, ops, o["dxb"].v, M, D)
    assert torch.equal(o["q"].v, q_ref), "bytes differ from vipant_quant_e4m3_mx of dx_bf16"
    assert torch.equal(mx_scales(ops, o["qs"].v, M, D), s_ref), "scales differ from vipant_quant_e4m3_mx of dx_bf16"


@pytest.mark.parametrize("x16", [False, True], ids=["x32", "x16"])
@pytest.mark.parametrize("M", [1, 5, 37])
def test_backward_f32dy_q8(ffi, ops, M, x16):
    """fp32 dy with q / qscale (compiled, no caller): the e4m3 form of the bf16 rounding of dx_f32."""
    D = 256
    o, _ = run_bwd_twice(ffi, D, M, "f32dy", x16, q=True)
    base, _ = run_bwd(ffi, D, M, "f32dy", x16, q=False)
    for k in base:
        assert torch.equal(o[k].parent, base[k].parent), f"{k}: the call with q differs from the call without"
    q_ref, s_ref = quantised_alone(ffi, ops, o["dx"].v[:, :D].to(BF16), M, D)
    assert torch.equal(o["q"].v, q_ref) and torch.equal(mx_scales(ops, o["qs"].v, M, D), s_ref)


# ------------------------------------------------------------------------------------------------------------------------ refusals
# name -> (entry point, what to change in its valid argument list, return code); t: the tensors of the test
REFUSALS = {
    "fwd_q_without_qscale": ("fwd", lambda a, t: a.update(q=t["q"].ptr()), EBADSHAPE),
    "fwd_qscale_without_q": ("fwd", lambda a, t: a.update(qs=t["qs"].ptr()), EBADSHAPE),
    "bwd_q_without_qscale": ("bwd", lambda a, t: a.update(q=t["q"].ptr()), EBADSHAPE),
    "bwd_qscale_without_q": ("bwd", lambda a, t: a.update(qs=t["qs"].ptr()), EBADSHAPE),
    "fwd_no_rows": ("fwd", lambda a, t: a.update(M=0), EBADSHAPE),
    "bwd_no_rows": ("bwd", lambda a, t: a.update(M=0), EBADSHAPE),
    "fwd_ldx_short": ("fwd", lambda a, t: a.update(ldx=a["D"] - 4), EALIGN),
    "fwd_ldx_odd": ("fwd", lambda a, t: a.update(ldx=a["D"] + 2), EALIGN),
    "bwd_ldx_short": ("bwd", lambda a, t: a.update(ldx=a["D"] - 4), EALIGN),
    "bwd_ldx_odd": ("bwd", lambda a, t: a.update(ldx=a["D"] + 2), EALIGN),
    "bwd_lddx_short": ("bwd", lambda a, t: a.update(lddx=a["D"] - 4), EALIGN),
    "bwd_lddx_odd": ("bwd", lambda a, t: a.update(lddx=a["D"] + 2), EALIGN),
    "fwd_x_f32_off_16_bytes": ("fwd", lambda a, t: a.update(x=t["x"].data_ptr() + 8), EALIGN),
    "fwd_x_f16_off_8_bytes": ("fwd", lambda a, t: a.update(x=t["x16"].data_ptr() + 4, flags=1), EALIGN),
    "bwd_no_workspace": ("bwd", lambda a, t: a.update(ws=None), ENOWORKSPACE),
    "bwd_workspace_one_byte_short": ("bwd", lambda a, t: a.update(wsn=a["wsn"] - 1), ENOWORKSPACE),
    "bwd_bf16_dres_missing": ("bwd", lambda a, t: a.update(flags=2), EBADSHAPE),
    "bwd_bf16_dres_with_f32_dy": ("bwd", lambda a, t: a.update(flags=3, dres=t["dres16"].data_ptr(), dy=t["dy32"].data_ptr()), EBADSHAPE),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_write_nothing(ffi, name):
    """Each VIPANT_REQUIRE of the two entry points beyond the width: its code, vipant_last_error() naming the entry point, and no output
    or workspace byte written.  (Every argument besides the refused one is valid; none of these reaches a kernel.)"""
    assert (ffi.STREAM_IN_F16, ffi.LN_DY_F32, ffi.LN_DRES_BF16) == (1, 1, 2)
    D, M = 256, 5
    entry, change, code = REFUSALS[name]
    t = dict(x=torch.ones(M + 1, D, device=DEV), x16=torch.ones(M + 1, D, dtype=F16, device=DEV), vec=torch.ones(D, device=DEV),
             stat=torch.ones(M, device=DEV), dy=torch.ones(M, D, dtype=BF16, device=DEV), dy32=torch.ones(M, D, device=DEV),
             dres16=torch.ones(M, D, dtype=BF16, device=DEV), q=G((M, D), U8), qs=G((ffi.query("vipant_mx_scale_bytes", M, D),), U8))
    o = dict(y=G((M, D), BF16), y32=G((M, D), F32), mean=G((M,), F32), rstd=G((M,), F32), sum=G((M, D), F32), dx=G((M, D), F32),
             dxb=G((M, D), BF16), dg=G((D,), F32), db=G((D,), F32), dcs=G((D,), F32), q=t["q"], qs=t["qs"])
    nbytes = ffi.query("vipant_layernorm_bwd_workspace_bytes", M, D)
    ws = Workspace(nbytes, DEV)
    L = ffi.lib()
    if entry == "fwd":
        a = dict(x=t["x"].data_ptr(), ldx=D, gamma=t["vec"].data_ptr(), beta=t["vec"].data_ptr(), y=o["y"].ptr(), y32=o["y32"].ptr(),
                 mean=o["mean"].ptr(), rstd=o["rstd"].ptr(), M=M, D=D, add=None, sum=None, q=None, qs=None, flags=0)
        change(a, t)
        rc = L.vipant_layernorm_fwd(*a.values(), st())
        want = b"layernorm_fwd"
    else:
        a = dict(dy=t["dy"].data_ptr(), flags=0, x=t["x"].data_ptr(), ldx=D, mean=t["stat"].data_ptr(), rstd=t["stat"].data_ptr(),
                 gamma=t["vec"].data_ptr(), dres=None, dx=o["dx"].ptr(), lddx=D, dxb=o["dxb"].ptr(), dg=o["dg"].ptr(), db=o["db"].ptr(),
                 dcs=o["dcs"].ptr(), acc=0, M=M, D=D, ws=ws.ptr(), wsn=nbytes, q=None, qs=None)
        change(a, t)
        rc = L.vipant_layernorm_bwd(*a.values(), st())
        want = b"layernorm_bwd"
    torch.cuda.synchronize()
    assert rc == code, (rc, L.vipant_last_error())
    assert want in L.vipant_last_error(), L.vipant_last_error()
    ws.untouched(f"{name}: refused")
    for k, v in o.items():
        v.untouched(f"{name}: {k}")
