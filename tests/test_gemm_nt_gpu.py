"""Parity of the NT contraction -- vipant_gemm_nt and vipant_gemm_nt_e4m3 (vipant_amd/csrc/gemm_nt.hip) -- over every kernel instance
the selector (nt_select.h) can pick, on both tile walks, at the edges and strides its callers can reach, against fp64 on the device.

The case lists live in tests/nt_cases.py; tests/test_nt_cases_cpu.py ties every case to the instance it claims (the selector driver)
and every row of NT_PP_INSTANCES, NT_PLAIN_INSTANCES and NT_FEW_ROWS_INSTANCES to a case, each bf16 ping-pong row on both walks.

Out of scope: vipant_gemm_nt_heads and vipant_gemm_nt_tokens (their own tests; the tokens path belongs to the token-boundary
operators), the device-only switches SKIP_STORES, E4M3_*_UNPAIRED and SINGLE_DRAWS, and TWO_STAGE.

LAYOUT.  A and B are views into larger parents: tight, padded to lda, ldb > K, or offset by a 16-byte-aligned column (what the block
backward passes: dqkv[:, D:]).  72 rows behind M (in A) and behind N (in B) and all padding columns hold NaN: rows out of range must
come back as zeros from the buffer descriptor (the few-rows kernel clamps the row index instead).  e4m3 operands are contiguous (the
scale layout is tied to the row length); their rows behind M hold the byte 0x7E (448) and the slots of those rows in the last 128-row
scale panel 0xFE.  C, aux, cq and the scales of cq are views into sentinel-filled parents -- 80 guard rows on both sides, padding
columns up to ldc, guard bytes around the scales and the scale slots of rows at and beyond M -- checked after every call; inputs
handed over as aux must come back unchanged.

  a. exact sweep.  A holds integers in -3..3, B integers in -3..3 times 2^-5 (pre-activations of standard deviation 2 at K = 256: the
     QuickGELU' codes span their range), bias and residual multiples of 2^-5.  Every product, every partial sum in any order and
     acc + bias are exact in fp32, so F32, SCALE_F32 (alpha = 1/4) and RESIDUAL_F32 must equal the fp64 result BIT FOR BIT, BF16 and the
     `u` output of QUICKGELU the round-to-nearest-even bf16 of it (f32x4_to_bf16x4 is the compiler's conversion, which rounds to
     nearest even).  A skipped, doubled, shifted or permuted row, column, K-tile or tile is a mismatch with no tolerance.  Outputs
     behind the gate, with u_b the exactly known input of the gate (the bf16 pre-activation on the ping-pong and few-rows kernels,
     the fp32 value on the plain kernel):
       g      within one bf16 rounding (unit roundoff 2^-8: eight significant bits) of the fp64 u_b sigmoid(1.702 u_b), plus 64 x 2^-23
              relative for the gate's fp32 arithmetic (nt_cases.GATE), plus 2^-126 (1 + |u_b|) absolute: v_rcp_f32 flushes a subnormal
              gate to zero (u_b below -51: reached by the Gaussian sweep only);
       codes  |code - (QuickGELU'(u_b) + 0.1) 212.5| <= 0.5 + 0.01 (nt_cases.CODE_SLACK);
       DQUICKGELU_D8   within one bf16 rounding of x (code / 212.5 - 0.1) in fp64, x = bf16(acc) on the ping-pong kernels (they stage the
              accumulator as bf16), x = acc on the few-rows kernel; the codes are random bytes, 0 and 255 included.  The decode
              itself runs in fp32 -- the constant 1 / 212.5, a product, the constant 0.1, a difference, on values below 1.2 --:
              4 x 2^-24 |x| absolute (nt_cases.DECODE), which matters only next to the zero of the decode (codes 21, 22), and 2^-24
              relative for the product with x;
       DQUICKGELU      likewise against x QuickGELU'(u) of the given bf16 u; the gate's budget enters as 64 x 2^-23 |x| ABSOLUTE, since
              QuickGELU' has a zero and its terms are of magnitude one.
  b. Gaussian sweep.  N(0, 1) 2^e with e per row in -6..6.  The budget is derived, not measured: products of two bf16 numbers are exact
     in fp32, so all error comes from additions, at most depth x 2^-23 x (|A| |B|^T + |bias| (+ |residual|)) =: E with depth the longest
     chain of additions (nt_cases.depth: 32 for the products of one v_mfma_f32_16x16x32_bf16, K / 32 accumulator steps, 1 for the bias,
     3 on the few-rows kernel for four waves' partial tiles, 1 for a residual, 1 for SCALE_F32's multiplication) and 2^-23 rather
     than 2^-24 because the matrix unit's adder may truncate.  On top of E come the output roundings of (a) with the gate's Lipschitz
     constants: the gate's input is known to du = E + 2^-8 (|u| + E) (E alone on the plain kernel; 0 where the launch hands u out, which
     is then checked against the reference by itself), g moves by at most 1.1 du, a code by 212.5 x 0.851 du.
  c. ticket walk.  Every ticket case three ways -- under STATIC_WALK, on tickets, and on tickets AGAIN directly behind a ticket launch
     of another shape (the ticket block must be back at zero, the two counter sets alternate): bit-identical, and a and b hold.  No
     CU-holding probe here; tests/test_kernels_gpu.py keeps that.
  d. e4m3.  The bf16 result against the fp64 product of the dequantised operands within 2^-8 of its row's largest element (the budget
     of tests/test_fp8_gpu.py, unchanged: the instruction's adder keeps fewer bits than fp32, no exactness); g, the codes and
     QuickGELU' from the codes as in (b) with du = that budget.  Every emit mode: the bytes and scales are what
     check_block_uniform_form (tests/mx_emul.py) demands of the bf16 result at slack 2; ALSO, ALONE and WITH_CODES agree bit for bit on
     everything they share, and so do the grouped and the plain walk (E4M3_EMIT_PLAIN_WALK, E4M3_WIDE_PLAIN_WALK).  emit8 writes bytes
     and scale bytes for rows below M only: the scale slots of rows at and beyond M stay sentinel, the last 32-row block's included,
     and the scales of a block that straddles M are within the slack of what its rows below M need.
  e. refusals return VIPANT_EBADSHAPE and write nothing.

The worst error / bound ratio of every case is printed, and written to the file VIPANT_NT_PARITY_LOG names if it is set
(profiles/nt_parity_observed.txt is one such run), so that a later change can tighten the bounds with evidence."""
import os

import pytest
import torch

import nt_cases as C
from mx_emul import check_block_uniform_form, dequant, dequant_mx, mx_scales

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
FILL = -1984.0           # sentinel of the bf16 and fp32 outputs (exact in bf16)
FILL8 = 0xA5             # sentinel of the byte outputs
GUARD = 80               # sentinel rows on both sides of an output (a multiple of 16: the views keep the parents' alignment)
POISON_ROWS = 72
ROW_BLOCK = 16384        # rows of the fp64 reference taken at a time
EBADSHAPE = -1
OBSERVED = []


@pytest.fixture(scope="module")
def ops():
    from vipant_amd import _ffi, ops as O
    _ffi.call("vipant_device_check")
    yield O
    path = os.environ.get("VIPANT_NT_PARITY_LOG")
    if OBSERVED and path:
        with open(path, "w") as f:
            f.write("# worst error / bound per case and output (tests/test_gemm_nt_gpu.py): exact sweep | Gaussian sweep\n")
            f.write("".join(line + "\n" for line in OBSERVED))


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def seed_of(c, salt=0):
    return ((c.M * 1000003 + c.N * 1009 + c.K) * 8 + c.epi) * 4 + salt


def stream():
    return torch.cuda.current_stream().cuda_stream


def place(data, ld, off, poison):
    """`data` as a view into a parent of row length `ld` whose other elements -- POISON_ROWS rows behind the last one, the columns in
    front of `off` and behind the data -- are `poison`."""
    M, N = data.shape
    parent = torch.full((M + POISON_ROWS, ld), poison, dtype=data.dtype, device=DEV)
    view = parent[:M, off:off + N]
    view.copy_(data)
    return view


class Box:
    """[M, N] as a view into a parent of row length ld filled with a sentinel, GUARD rows on both sides."""

    def __init__(self, M, N, ld, off, dtype, init=None):
        self.fill = FILL8 if dtype == torch.uint8 else FILL
        self.parent = torch.full((M + 2 * GUARD, ld), self.fill, dtype=dtype, device=DEV)
        self.M, self.N, self.ld, self.off = M, N, ld, off
        self.v = self.parent[GUARD:GUARD + M, off:off + N]
        if init is not None:
            self.v.copy_(init)

    def ptr(self):
        return self.v.data_ptr()

    def intact_around(self, what):
        p, f = self.parent, self.fill
        ok = bool((p[:GUARD] == f).all()) and bool((p[GUARD + self.M:] == f).all())
        if self.off:
            ok = ok and bool((p[GUARD:GUARD + self.M, :self.off] == f).all())
        if self.off + self.N < self.ld:
            ok = ok and bool((p[GUARD:GUARD + self.M, self.off + self.N:] == f).all())
        assert ok, f"{what}: written outside its [{self.M}, {self.N}] box (ld {self.ld}, offset {self.off})"

    def untouched(self, what):
        assert bool((self.parent == self.fill).all()), f"{what}: written"


def ratio(got, ref, bound):
    """Worst |got - ref| / bound; inf where a zero bound is missed; NaN where the output is."""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = torch.where(torch.isnan(err), torch.full_like(err, NAN), r)
    return float(r.max()) if r.numel() else 0.0


def quickgelu(u):
    return u * torch.sigmoid(1.702 * u)


def quickgelu_prime(u):
    sg = torch.sigmoid(1.702 * u)
    return sg * (1 + 1.702 * u * (1 - sg))


def rne_bf16(x):
    """fp64 values that fp32 holds exactly -> their round-to-nearest-even bf16 (torch's conversion), as fp64."""
    return x.float().to(torch.bfloat16).double()


# ------------------------------------------------------------------------------------------------------------------- bf16 operands
OUT_DTYPE = {C.BF16: torch.bfloat16, C.F32: torch.float32, C.RESIDUAL_F32: torch.float32, C.QUICKGELU: torch.bfloat16,
             C.DQUICKGELU: torch.bfloat16, C.SCALE_F32: torch.float32, C.QUICKGELU_D8: torch.bfloat16, C.DQUICKGELU_D8: torch.bfloat16}
AUX_DTYPE = {C.RESIDUAL_F32: torch.float32, C.QUICKGELU: torch.bfloat16, C.DQUICKGELU: torch.bfloat16, C.QUICKGELU_D8: torch.uint8,
             C.DQUICKGELU_D8: torch.uint8}
AUX_IS_INPUT = (C.RESIDUAL_F32, C.DQUICKGELU, C.DQUICKGELU_D8)
NO_BIAS = (C.DQUICKGELU, C.DQUICKGELU_D8, C.SCALE_F32)        # the epilogues that read none


class Data:
    """Operands of one case: a, b (contiguous data), av, bv (the views the launch gets), bias, aux_in, alpha."""


def operands(c, exact):
    lda, ldb, _, oa, ob, _ = C.layout(c)
    g = gen(seed_of(c, 0 if exact else 1))
    d = Data()
    d.exact = exact
    if exact:
        d.a = torch.randint(-3, 4, (c.M, c.K), generator=g, device=DEV).to(torch.bfloat16)
        d.b = (torch.randint(-3, 4, (c.N, c.K), generator=g, device=DEV).float() / 32).to(torch.bfloat16)
        d.bias = torch.randint(-64, 65, (c.N,), generator=g, device=DEV).float() / 32
        res = torch.randint(-256, 257, (c.M, c.N), generator=g, device=DEV).float() / 32
        d.alpha = 0.25
    else:
        ea = torch.exp2(torch.randint(-6, 7, (c.M, 1), generator=g, device=DEV).float())
        eb = torch.exp2(torch.randint(-6, 7, (c.N, 1), generator=g, device=DEV).float())
        d.a = (torch.randn(c.M, c.K, generator=g, device=DEV) * ea).to(torch.bfloat16)
        d.b = (torch.randn(c.N, c.K, generator=g, device=DEV) * eb * c.K ** -0.5).to(torch.bfloat16)
        d.bias = torch.randn(c.N, generator=g, device=DEV)
        res = torch.randn(c.M, c.N, generator=g, device=DEV) * ea
        d.alpha = 0.37
    d.av, d.bv = place(d.a, lda, oa, NAN), place(d.b, ldb, ob, NAN)
    d.aux_in = None
    if c.epi == C.RESIDUAL_F32:
        d.aux_in = res
    elif c.epi == C.DQUICKGELU:
        d.aux_in = (torch.randn(c.M, c.N, generator=g, device=DEV) * 2).to(torch.bfloat16)
    elif c.epi == C.DQUICKGELU_D8:
        d.aux_in = torch.randint(0, 256, (c.M, c.N), generator=g, device=DEV, dtype=torch.uint8)
        d.aux_in[0, 0], d.aux_in[-1, -1] = 0, 255
    if c.epi in NO_BIAS:
        d.bias = None
    return d


def launch(ops, c, d, what, sw=None, aux_shift=0, expect_refusal=False):
    """One vipant_gemm_nt call of case `c` on the operands `d` under the switches `sw` (default: the case's).  Returns (C, aux) boxes
    after checking everything around them.  `aux_shift`: bytes added to the pointer of aux (a misaligned code matrix)."""
    from vipant_amd import _ffi
    _, _, ldc, _, _, oc = C.layout(c)
    os.environ["VIPANT_GEMM_VARIANT"] = str(c.sw if sw is None else sw)
    out = Box(c.M, c.N, ldc, oc, OUT_DTYPE[c.epi], init=d.aux_in if c.inplace else None)
    aux = None
    if c.epi in AUX_DTYPE and not c.inplace:
        aux = Box(c.M, c.N, ldc, oc, AUX_DTYPE[c.epi], init=d.aux_in if c.epi in AUX_IS_INPUT else None)
    aux_ptr = out.ptr() if c.inplace else (aux.ptr() + aux_shift if aux is not None else None)
    args = (d.av.data_ptr(), d.av.stride(0), d.bv.data_ptr(), d.bv.stride(0), out.ptr(), ldc, d.bias.data_ptr() if d.bias is not None else None,
            aux_ptr, float(d.alpha), c.M, c.N, c.K, c.epi | (_ffi.EPI_FEW_ROWS if c.few else 0), stream())
    if expect_refusal:
        rc = getattr(_ffi.lib(), "vipant_gemm_nt")(*args)
        torch.cuda.synchronize()
        assert rc == EBADSHAPE, f"{what}: returned {rc}, not VIPANT_EBADSHAPE"
        out.untouched(what + ": C")
        if aux is not None and c.epi in AUX_IS_INPUT:
            aux.intact_around(what + ": aux")
            assert torch.equal(aux.v, d.aux_in), f"{what}: the aux input was changed"
        elif aux is not None:
            aux.untouched(what + ": aux")
        return out, aux
    ops.call("vipant_gemm_nt", *args)
    out.intact_around(what + ": C")
    if aux is not None:
        aux.intact_around(what + ": aux")
        if c.epi in AUX_IS_INPUT:
            assert torch.equal(aux.v, d.aux_in), f"{what}: the aux input was changed"
    return out, aux


def verify(c, d, out, aux, what):
    """Parts a and b of the module docstring for one launch's outputs; returns {output name: worst error / bound}."""
    fam = C.parse_instance(c.inst)[0]
    exact = d.exact
    depth = C.depth(c)
    worst = {}

    def note(name, r):
        worst[name] = max(worst.get(name, 0.0), r) if r == r else NAN

    bd, biasd = d.b.double(), (d.bias.double() if d.bias is not None else None)
    for lo in range(0, c.M, ROW_BLOCK):
        hi = min(c.M, lo + ROW_BLOCK)
        ad = d.a[lo:hi].double()
        acc = ad @ bd.t()
        got = out.v[lo:hi]
        aux_in = d.aux_in[lo:hi] if d.aux_in is not None else None
        if exact:
            assert float(acc.abs().max()) * 32 < 2 ** 24
            E0 = E = torch.zeros_like(acc)
        else:
            mag = ad.abs() @ bd.abs().t()
            E0 = depth * C.U32 * mag
            E = depth * C.U32 * (mag + (biasd.abs() if biasd is not None else 0) + (aux_in.double().abs() if c.epi == C.RESIDUAL_F32 else 0))
        pre = acc + biasd if biasd is not None else acc
        rounded = lambda v, e: e + C.U16 * (v.abs() + e)          # e, then one rounding to bf16
        if c.epi == C.F32:
            note("C", ratio(got, pre, E))
        elif c.epi == C.SCALE_F32:
            note("C", ratio(got, d.alpha * acc, abs(d.alpha) * E))
        elif c.epi == C.RESIDUAL_F32:
            note("C", ratio(got, pre + aux_in.double(), E))
        elif c.epi == C.BF16:
            note("C", ratio(got, rne_bf16(pre), E) if exact else ratio(got, pre, rounded(pre, E)))
        elif c.epi in (C.QUICKGELU, C.QUICKGELU_D8):
            if c.epi == C.QUICKGELU:
                u = aux.v[lo:hi]
                note("u", ratio(u, rne_bf16(pre), E) if exact else ratio(u, pre, rounded(pre, E)))
            # the gate's input: exactly known in the exact sweep; in the Gaussian sweep the u the launch handed out (ping-pong and
            # few-rows kernels: the gate sees exactly that), else the reference within du
            if fam == "plain":
                ub, du = pre, E
            elif exact:
                ub, du = rne_bf16(pre), E
            elif c.epi == C.QUICKGELU:
                ub, du = aux.v[lo:hi].double(), torch.zeros_like(E)
            else:
                ub, du = pre, rounded(pre, E)
            g_ref = quickgelu(ub)
            note("g", ratio(got, g_ref, C.LIP_G * du + (C.U16 + C.GATE) * (g_ref.abs() + C.LIP_G * du) + C.FLUSH * (1 + ub.abs())))
            if c.epi == C.QUICKGELU_D8:
                note("code", ratio(aux.v[lo:hi], (quickgelu_prime(ub) + 0.1) * 212.5, C.CODE_SLACK + 212.5 * C.LIP_CODE * du))
        else:       # the two backward epilogues: x times a derivative
            if fam == "pingpong":        # the accumulator is staged as bf16
                x, dx = (rne_bf16(acc), E0) if exact else (acc, rounded(acc, E0))
            else:
                x, dx = acc, E0
            if c.epi == C.DQUICKGELU_D8:
                dg = aux_in.double() / 212.5 - 0.1
                arith = C.DECODE * (x.abs() + dx) + 2.0 ** -24 * (x * dg).abs()
            else:
                dg = quickgelu_prime(aux_in.double())
                arith = C.GATE * (x.abs() + dx)
            ref = x * dg
            note("C", ratio(got, ref, dg.abs() * dx + C.U16 * (ref.abs() + dg.abs() * dx) + arith))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, f"{what} {C.case_id(c)} -> {c.inst}: error / bound {bad} ({'exact' if exact else 'Gaussian'} sweep, depth {depth})"
    return worst


def record(c, we, wg, tag=""):
    names = sorted(set(we) | set(wg))
    line = "gemm_nt%s %-46s %-50s depth %3d: " % (tag, C.case_id(c), c.inst, C.depth(c)) + "  ".join(
        "%s %.4f | %.4f" % (k, we.get(k, 0.0), wg.get(k, 0.0)) for k in names)
    print(line)
    OBSERVED.append(line)


def both_sweeps(ops, c):
    w = []
    for exact in (True, False):
        d = operands(c, exact)
        out, aux = launch(ops, c, d, "exact" if exact else "gaussian")
        w.append(verify(c, d, out, aux, "exact" if exact else "gaussian"))
        if c.few and c.epi == C.BF16 and c.M >= 63:
            # one row's result is bit-identical inside a smaller launch (what `running.micro_batch` relies on)
            sub = c._replace(M=33)
            ds = Data()
            ds.exact, ds.alpha, ds.bias, ds.aux_in = exact, d.alpha, d.bias, None
            ds.a, ds.b, ds.av, ds.bv = d.a[7:40], d.b, d.av[7:40], d.bv
            o2, _ = launch(ops, sub, ds, "rows 7..39 alone")
            assert torch.equal(o2.v, out.v[7:40]), f"{C.case_id(c)}: a row's result depends on the rows that travel with it"
    record(c, w[0], w[1])


def by_instance(cases):
    groups = {}
    for c in cases:
        groups.setdefault(c.inst, []).append(c)
    return sorted(groups.items())


@pytest.fixture
def switches():
    """The library reads VIPANT_GEMM_VARIANT on every call; launch() sets it per case."""
    before = os.environ.get("VIPANT_GEMM_VARIANT")
    yield
    if before is None:
        os.environ.pop("VIPANT_GEMM_VARIANT", None)
    else:
        os.environ["VIPANT_GEMM_VARIANT"] = before


@pytest.mark.parametrize("inst,cases", by_instance(C.STATIC_CASES), ids=[i.replace(" ", ",") for i, _ in by_instance(C.STATIC_CASES)])
def test_static_walk_over_more_than_256_tiles(ops, switches, inst, cases):
    """a, b.  258 tiles and short K: the K-tile stream wraps from tile to tile; two to nine and sixteen K-tiles on every schedule, the
    grouped walk with every remainder of the row-tile count, both store paths of QUICKGELU_D8, ragged last column tiles."""
    for c in cases:
        both_sweeps(ops, c)


@pytest.mark.parametrize("inst,cases", by_instance(C.SMALL_CASES), ids=[i.replace(" ", ",") for i, _ in by_instance(C.SMALL_CASES)])
def test_fewer_than_256_tiles(ops, switches, inst, cases):
    """a, b.  One to three tiles and nine (a grid of 16), M and N on either side of the tile and of a wave group's 128 rows."""
    for c in cases:
        both_sweeps(ops, c)


@pytest.mark.parametrize("inst,cases", by_instance(C.PLAIN_CASES), ids=[i.replace(" ", ",") for i, _ in by_instance(C.PLAIN_CASES)])
def test_plain_kernel(ops, switches, inst, cases):
    """a, b.  K = 64, N % 8 == 4, ldc % 8 == 4, the fp32 epilogues at K = 64 and 1024, RESIDUAL_F32 in place and not, SCALE_F32."""
    for c in cases:
        both_sweeps(ops, c)


@pytest.mark.parametrize("inst,cases", by_instance(C.FEW_ROWS_CASES), ids=[i.replace(" ", ",") for i, _ in by_instance(C.FEW_ROWS_CASES)])
def test_few_rows_kernel(ops, switches, inst, cases):
    """a, b.  K over the period of 768 (four waves x six K-steps of 32) and K = 64 (three waves idle); M and N around the 64 x 64 tile;
    a row's result is bit-identical inside a smaller launch."""
    for c in cases:
        both_sweeps(ops, c)


# ------------------------------------------------------------------------------------------------------------------- c
TICKET_PAIRS = list(zip(C.TICKET_CASES[0::2], C.TICKET_CASES[1::2]))


@pytest.mark.parametrize("case,twin", TICKET_PAIRS, ids=[C.case_id(c) for c, _ in TICKET_PAIRS])
def test_ticket_walk(ops, switches, case, twin):
    """c.  Static walk, tickets, tickets again behind a ticket launch of another shape: bit-identical, and a and b hold."""
    other = C.TICKET_NEIGHBOURS[0] if case.N != C.TICKET_NEIGHBOURS[0].N else C.TICKET_NEIGHBOURS[1]
    do = operands(other, True)
    w = []
    for exact in (True, False):
        d = operands(case, exact)
        s_out, s_aux = launch(ops, twin, d, "static walk")
        t_out, t_aux = launch(ops, case, d, "ticket walk")
        launch(ops, other, do, "another shape on tickets")
        r_out, r_aux = launch(ops, case, d, "ticket walk, again")
        # each of the three against the reference (a, b), then bit for bit against each other
        w.append(verify(twin, d, s_out, s_aux, "static walk"))
        verify(case, d, t_out, t_aux, "ticket walk")
        verify(case, d, r_out, r_aux, "ticket walk behind another ticket launch")
        for name, (o, a) in (("tickets", (t_out, t_aux)), ("tickets behind another ticket launch", (r_out, r_aux))):
            assert torch.equal(o.v, s_out.v), f"{C.case_id(case)}: C on {name} differs from the static walk"
            assert a is None or torch.equal(a.v, s_aux.v), f"{C.case_id(case)}: aux on {name} differs from the static walk"
        del s_out, s_aux, t_out, t_aux, r_out, r_aux, d
    record(case, w[0], w[1], tag=" (static = tickets = tickets again)")


# ------------------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("case,why", C.REFUSALS, ids=[w.replace(" ", "_") + f"-e{c.epi}" for c, w in C.REFUSALS])
def test_refusals_write_nothing(ops, switches, case, why):
    d = operands(case, True)
    launch(ops, case, d, why, expect_refusal=True)


@pytest.mark.parametrize("case,refusal,why", C.MISALIGNED_AUX, ids=[w.replace(" ", "_") + f"-e{c.epi}" for c, _, w in C.MISALIGNED_AUX])
def test_misaligned_aux_is_refused(ops, switches, case, refusal, why):
    d = operands(case, True)
    launch(ops, case, d, why, aux_shift=8, expect_refusal=True)
    out, aux = launch(ops, case, d, why + ", aligned")           # the same launch with an aligned aux runs
    verify(case, d, out, aux, why + ", aligned")


# ------------------------------------------------------------------------------------------------------------------- d
E4M3_POISON, SCALE_POISON = 0x7E, 0xFE


def e4m3_shapes():
    groups = {}
    for c in C.E4M3_CASES:
        groups.setdefault((c.M, c.N, c.K), []).append(c)
    return sorted(groups.items())


class ScaleBox:
    """The MX scales of an emitted [M, N] form between two guard zones; every byte starts as the sentinel."""

    def __init__(self, ops, M, N):
        self.n = ops.query("vipant_mx_scale_bytes", M, N)
        self.buf = torch.full((self.n + 512,), FILL8, dtype=torch.uint8, device=DEV)
        self.v = self.buf[256:256 + self.n]
        Mp = C.ceil_div(M, 128) * 128
        self.beyond = ops.mx_scale_index(Mp, N, DEV)[M:].reshape(-1)        # the slots of rows at and beyond M

    def check(self, what):
        assert bool((self.buf[:256] == FILL8).all()) and bool((self.buf[256 + self.n:] == FILL8).all()), f"{what}: written around the scales"
        assert bool((self.v[self.beyond] == FILL8).all()), f"{what}: scale bytes written for rows at and beyond M"


@pytest.mark.parametrize("shape,cases", e4m3_shapes(), ids=["%dx%dx%d" % s for s, _ in e4m3_shapes()])
def test_e4m3(ops, switches, shape, cases):
    """d.  Every e4m3 instance that a launch of this shape reaches, on one set of operands."""
    M, N, K = shape
    g = gen(seed_of(cases[0], 2))
    a_unit = torch.randn(M, K, generator=g, device=DEV)
    b_unit = torch.randn(N, K, generator=g, device=DEV) * K ** -0.5
    ea = torch.exp2(torch.randint(-6, 7, (M, 1), generator=g, device=DEV).float())
    eb = torch.exp2(torch.randint(-6, 7, (N, 1), generator=g, device=DEV).float())
    bias = torch.randn(N, generator=g, device=DEV)
    codes_in = torch.randint(0, 256, (M, N), generator=g, device=DEV, dtype=torch.uint8)
    codes_in[0, 0], codes_in[-1, -1] = 0, 255
    operand_sets = {}

    def quantised(spread):
        """(A view, its scales, B view, its scales, the fp64 product of the dequantised operands); `spread`: rows over 12 binades and one
        block of every row 32 times larger (the plain epilogue, as tests/test_fp8_gpu.py); else unit scale (the QuickGELU epilogues)."""
        if spread not in operand_sets:
            a = (a_unit * ea if spread else a_unit).to(torch.bfloat16)
            b = (b_unit * eb if spread else b_unit).to(torch.bfloat16)
            if spread:
                a[:, 64:96] *= 32.0
            pa = torch.full((M + POISON_ROWS, K), E4M3_POISON, dtype=torch.uint8, device=DEV)
            pb = torch.full((N + POISON_ROWS, K), E4M3_POISON, dtype=torch.uint8, device=DEV)
            sa = torch.full((ops.query("vipant_mx_scale_bytes", M, K),), SCALE_POISON, dtype=torch.uint8, device=DEV)
            sb = torch.empty(N, dtype=torch.uint8, device=DEV)
            ops.quant_e4m3_mx(a, q=pa[:M], scale=sa)
            ops.quant_e4m3(b, q=pb[:N], scale=sb)
            sa[ops.mx_scale_index(C.ceil_div(M, 128) * 128, K, DEV)[M:].reshape(-1)] = SCALE_POISON
            assert bool((pa[M:] == E4M3_POISON).all()) and bool((pb[N:] == E4M3_POISON).all())
            acc = dequant_mx(ops, pa[:M], sa).double() @ dequant(pb[:N], sb).double().t()
            operand_sets[spread] = (pa[:M], sa, pb[:N], sb, acc)
        return operand_sets[spread]

    results = {}
    for c in cases:
        _, _, ldc, _, _, oc = C.layout(c)
        _, _, sched, _, emit, _ = C.parse_instance(c.inst)
        qa, sa, qb, sb, acc = quantised(c.epi == C.BF16)
        os.environ["VIPANT_GEMM_VARIANT"] = str(c.sw)
        what = C.case_id(c)
        out = None if c.c_null else Box(M, N, ldc, oc, torch.bfloat16)
        aux = None if c.aux_null else Box(M, N, ldc, oc, torch.uint8, init=codes_in if c.epi == C.DQUICKGELU_D8 else None)
        cq = None if c.cq_null else Box(M, N, N, 0, torch.uint8)
        cqs = None if c.cq_null else ScaleBox(ops, M, N)
        use_bias = c.epi != C.DQUICKGELU_D8
        ops.call("vipant_gemm_nt_e4m3", qa.data_ptr(), K, sa.data_ptr(), qb.data_ptr(), K, sb.data_ptr(), out.ptr() if out else None, ldc,
                 bias.data_ptr() if use_bias else None, aux.ptr() if aux else None, cq.ptr() if cq else None, cqs.v.data_ptr() if cqs else None,
                 M, N, K, c.epi, stream())
        for name, box in (("C", out), ("aux", aux), ("cq", cq)):
            if box is not None:
                box.intact_around(f"{what}: {name}")
        if cqs is not None:
            cqs.check(what)
        if c.epi == C.DQUICKGELU_D8:
            assert torch.equal(aux.v, codes_in), f"{what}: the codes were changed"
        results[c] = (out, aux, cq, cqs)
        # against the fp64 product of the dequantised operands
        w = {}
        pre = acc + bias.double() if use_bias else acc
        du = C.U16 * pre.abs().amax(dim=1, keepdim=True).expand_as(pre)
        if out is not None:
            if c.epi == C.BF16:
                w["C"] = ratio(out.v, pre, du)
            elif c.epi == C.QUICKGELU_D8:
                g_ref = quickgelu(pre)
                w["g"] = ratio(out.v, g_ref, C.LIP_G * du + (C.U16 + C.GATE) * (g_ref.abs() + C.LIP_G * du) + C.FLUSH * (1 + pre.abs()))
            else:
                dg = codes_in.double() / 212.5 - 0.1
                ref = pre * dg
                w["C"] = ratio(out.v, ref, dg.abs() * du + C.U16 * (ref.abs() + dg.abs() * du) + C.DECODE * (pre.abs() + du) + 2.0 ** -24 * ref.abs())
        if aux is not None and c.epi == C.QUICKGELU_D8:
            w["code"] = ratio(aux.v, (quickgelu_prime(pre) + 0.1) * 212.5, C.CODE_SLACK + 212.5 * C.LIP_CODE * du)
        line = "gemm_nt_e4m3 %-46s %-50s: " % (what, c.inst) + "  ".join("%s %.4f" % kv for kv in sorted(w.items()))
        print(line)
        OBSERVED.append(line)
        assert all(v <= 1.0 for v in w.values()), line
    # the emitted form is that of the bf16 result; every mode and both walks agree bit for bit on what they share
    for epi in (C.BF16, C.QUICKGELU_D8, C.DQUICKGELU_D8):
        mine = [(c, r) for c, r in results.items() if c.epi == epi]
        same_schedule = {}
        for c, r in mine:
            same_schedule.setdefault(C.parse_instance(c.inst)[2] in (C.DEEP, C.DEEP_GROUPED) if epi == C.BF16 else True, []).append((c, r))
        for group in same_schedule.values():
            for i, name in enumerate(("C", "aux", "cq")):
                have = [(c, r[i].v) for c, r in group if r[i] is not None]
                for c, v in have[1:]:
                    assert torch.equal(v, have[0][1]), f"{name} of {C.case_id(c)} differs from {C.case_id(have[0][0])}"
            have = [(c, mx_scales(ops, r[3].v, M, N)) for c, r in group if r[3] is not None]
            for c, v in have[1:]:
                assert torch.equal(v, have[0][1]), f"the emitted scales of {C.case_id(c)} differ from {C.case_id(have[0][0])}"
        also = [r for c, r in mine if C.parse_instance(c.inst)[4] == C.EMIT_ALSO]
        if also:
            out, _, cq, cqs = also[0]
            check_block_uniform_form(ops, (cq.v, cqs.v), out.v.contiguous(), slack=2)
        assert epi == C.BF16 or not any(r[2] is not None for _, r in mine) or also, "an emitted form without an ALSO launch to compare it with"
