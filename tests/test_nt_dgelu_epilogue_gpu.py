"""The QuickGELU' epilogues of the ping-pong NT kernels (VIPANT_EPI_DQUICKGELU_D8 from 8-bit codes, VIPANT_EPI_DQUICKGELU from bf16
pre-activations) request the inputs of all four store rounds of a tile in front of the tile's first store -- round 0's codes already in
the tile's last K-tile on the DEEP schedules -- and await them once.  A code taken from the wrong round, row or tile, or read before it
has arrived, is what these cases are for:

  tile wrap      M = 33 000, N = 1024, K = 192, DEEP: 516 tiles on 256 workgroups, every workgroup runs at least two, and the K-tile
                 stream (three K-tiles) wraps across an epilogue;
  grouped walk   M = 22 400, N = 3072, K = 128: DEEP on the column-grouped walk for the codes (the step's own instantiation; the bf16
                 pre-activation epilogue has no such instance and runs its default, the k-step schedule);
  edges          M = 300, N = 264, ldc = N + 40, K = 128: the last row tile has 44 live rows, the last column tile one live 8-column
                 chunk -- the bounds checks of loads and stores on both axes;
  tickets        M = 22 400, N = 3072, K = 256, codes only: the shapes above are too short (K < 256) for the library to draw tickets,
                 so with or without _ffi.SW_STATIC_WALK they run the static kernel; this one runs gemm_nt_pp_kernel<7, 12, 2, 0, true>.

Every case runs with the switches the walk asks for and once more with _ffi.SW_STATIC_WALK added.  Operands are views into NaN-filled
parents (anything read outside them poisons the result), the codes a view into a parent of other bytes, the output a view into a
sentinel-filled parent with guard rows.  Operands are integers in -3..3, so the accumulator is exact and x = bf16(acc) is known; the codes
are uniform in 0..255.  Checked:
  * the result lies within one bf16 rounding of x (code / 212.5 - 0.1) in fp64 -- the bound tests/test_gemm_nt_gpu.py states for this
    epilogue: U16 |ref| for the rounding, DECODE |x| + 2^-24 |ref| for the decode and the product in fp32 (nt_cases); for the bf16
    pre-activations: U16 |ref| + GATE |x|;
  * the walk's result equals the static walk's bit for bit, and a second launch equals the first bit for bit;
  * nothing around the output or the inputs is written, and the inputs are unchanged."""
import os

import pytest
import torch

import nt_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FILL = -1984.0           # sentinel of the output (exact in bf16)
CODE_FILL = 0x5A         # what surrounds the code matrix
GUARD = 80
ROW_BLOCK = 8192

# (name, M, N, K, ldc or 0, {epilogue: (switches, the instance the launch reaches without STATIC_WALK)})
SHAPES = [
    ("tile_wrap", 33000, 1024, 192, 0, {C.DQUICKGELU_D8: (C.DA, C.pp(C.DQUICKGELU_D8, C.DEEP)), C.DQUICKGELU: (C.DA, C.pp(C.DQUICKGELU, C.DEEP))}),
    ("grouped_walk", 22400, 3072, 128, 0, {C.DQUICKGELU_D8: (0, C.pp(C.DQUICKGELU_D8, C.DEEP_GROUPED)), C.DQUICKGELU: (0, C.pp(C.DQUICKGELU, C.KSTEP))}),
    ("edges", 300, 264, 128, 304, {C.DQUICKGELU_D8: (0, C.pp(C.DQUICKGELU_D8, C.DEEP)), C.DQUICKGELU: (0, C.pp(C.DQUICKGELU, C.KSTEP))}),
    ("tickets", 22400, 3072, 256, 0, {C.DQUICKGELU_D8: (0, C.pp(C.DQUICKGELU_D8, C.DEEP_GROUPED, ticket=1))}),
]
CASES = [(name, C.bf16_case(M, N, K, epi, inst, sw=sw, ldc=ldc)) for name, M, N, K, ldc, per in SHAPES for epi, (sw, inst) in per.items()]


@pytest.fixture(scope="module")
def ops():
    from vipant_amd import _ffi, ops as O
    _ffi.call("vipant_device_check")
    return O


@pytest.fixture
def switches():
    before = os.environ.get("VIPANT_GEMM_VARIANT")
    yield
    if before is None:
        os.environ.pop("VIPANT_GEMM_VARIANT", None)
    else:
        os.environ["VIPANT_GEMM_VARIANT"] = before


def boxed(data, ld, fill):
    """`data` as a view into a parent of row length `ld` filled with `fill`, GUARD rows on both sides: (parent, view)."""
    M, N = data.shape
    parent = torch.full((M + 2 * GUARD, ld), fill, dtype=data.dtype, device=DEV)
    view = parent[GUARD:GUARD + M, :N]
    view.copy_(data)
    return parent, view


def intact_around(parent, M, N, fill, what):
    same = (lambda t: t.isnan()) if fill != fill else (lambda t: t == fill)
    ok = bool(same(parent[:GUARD]).all()) and bool(same(parent[GUARD + M:]).all()) and bool(same(parent[GUARD:GUARD + M, N:]).all())
    assert ok, f"{what}: written outside its [{M}, {N}] box"


def launch(ops, c, sw, a, b, aux, ldc):
    os.environ["VIPANT_GEMM_VARIANT"] = str(sw)
    parent, out = boxed(torch.full((c.M, c.N), FILL, dtype=torch.bfloat16, device=DEV), ldc, FILL)
    ops.call("vipant_gemm_nt", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), ldc, None, aux.data_ptr(), 1.0,
             c.M, c.N, c.K, c.epi, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact_around(parent, c.M, c.N, FILL, f"{C.case_id(c)} switches {sw}: C")
    return out


@pytest.mark.parametrize("name,c", CASES, ids=[f"{n}-e{c.epi}" for n, c in CASES])
def test_quickgelu_derivative_epilogue(ops, switches, name, c):
    from vipant_amd import _ffi
    assert C.STATIC == _ffi.SW_STATIC_WALK
    g = torch.Generator(device=DEV)
    g.manual_seed((c.M * 1009 + c.N) * 8 + c.epi)
    a = torch.randint(-3, 4, (c.M, c.K), generator=g, device=DEV).to(torch.bfloat16)
    b = torch.randint(-3, 4, (c.N, c.K), generator=g, device=DEV).to(torch.bfloat16)
    ldc = C.layout(c)[2]
    ap, av = boxed(a, c.K + 8, NAN)
    bp, bv = boxed(b, c.K + 24, NAN)
    if c.epi == C.DQUICKGELU_D8:
        aux_in = torch.randint(0, 256, (c.M, c.N), generator=g, device=DEV, dtype=torch.uint8)
        aux_in[0, 0], aux_in[-1, -1] = 0, 255
        xp, aux = boxed(aux_in, ldc, CODE_FILL)
    else:
        aux_in = (torch.randn(c.M, c.N, generator=g, device=DEV) * 2).to(torch.bfloat16)
        xp, aux = boxed(aux_in, ldc, NAN)

    first = launch(ops, c, c.sw, av, bv, aux, ldc)
    second = launch(ops, c, c.sw, av, bv, aux, ldc)
    static = launch(ops, c, c.sw | C.STATIC, av, bv, aux, ldc)
    assert torch.equal(aux, aux_in), "the aux input was changed"
    intact_around(xp, c.M, c.N, CODE_FILL if c.epi == C.DQUICKGELU_D8 else NAN, "aux")
    intact_around(ap, c.M, c.K, NAN, "A")
    intact_around(bp, c.N, c.K, NAN, "B")

    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(second), bits(first)), "a second launch differs from the first"
    assert torch.equal(bits(static), bits(first)), "the walk's result differs from the static walk's"

    worst = 0.0
    bd = b.double()
    for lo in range(0, c.M, ROW_BLOCK):
        hi = min(c.M, lo + ROW_BLOCK)
        acc = a[lo:hi].double() @ bd.t()
        assert float(acc.abs().max()) < 2 ** 24
        x = acc.float().to(torch.bfloat16).double()              # the accumulator is exact and staged as bf16
        if c.epi == C.DQUICKGELU_D8:
            dg = aux_in[lo:hi].double() / 212.5 - 0.1
            ref = x * dg
            bound = C.U16 * ref.abs() + C.DECODE * x.abs() + 2.0 ** -24 * ref.abs()
        else:
            u = aux_in[lo:hi].double()
            sg = torch.sigmoid(1.702 * u)
            ref = x * (sg * (1 + 1.702 * u * (1 - sg)))
            bound = C.U16 * ref.abs() + C.GATE * x.abs()
        err = (first[lo:hi].double() - ref).abs()
        assert not bool(err.isnan().any()), f"{name}: NaN in the result (rows {lo}..{hi})"
        r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        worst = max(worst, float(r.max()))
    print(f"gemm_nt dgelu epilogue {name} {C.case_id(c)} -> {c.inst}: worst error / bound {worst:.4f}")
    assert worst <= 1.0, f"{name} {C.case_id(c)}: error / bound {worst}"
