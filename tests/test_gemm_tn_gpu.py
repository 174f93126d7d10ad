"""Parity of the weight-gradient contraction -- vipant_gemm_tn, vipant_gemm_tn_pair, vipant_gemm_tn_e4m3 (vipant_amd/csrc/gemm_tn.hip)
-- over every split plan, edge and stride its callers can reach, against fp64 on the device.

The case lists and the Python restatement of the split plans live in tests/tn_plan.py; tests/test_tn_plan_cpu.py ties the restatement
to the library and asserts what the lists cover: runs of 1..9 and 16 K-tiles per workgroup (the ping-pong stream's state has period
6 in the K-tile index), short last splits, every M tail, the direct path on one, four and sixteen K-tiles, the reduce kernels' grid
caps, every tail of the column-sum reduction loop, ragged P and Q.

Every operand is a VIEW into a larger parent whose other elements are NaN: the rows at and beyond M (the buffer descriptor must clip
them), the padding columns up to lda / ldb, and, for the layout "o", the columns in front of a 16-byte-aligned offset (what the block
backward passes: dqkv[:, D:] with lda = 3 D).  C and a_colsum are views into parents filled with a sentinel, the workspace is handed
over with exactly the byte count the query returned between two guard zones, and every call checks all of them.

  a. exact sweep: integer operands in -3..3.  Every product and every partial sum, in any order, is an integer below 2^24
     (9 M < 2^16), which fp32 represents exactly whatever the order or the adder's rounding: C and the column sums must equal the
     integer reference BIT FOR BIT.  No tolerance; a skipped, doubled, shifted or permuted row, column, K-tile or split is a mismatch.
  b. Gaussian sweep: N(0, 1) 2^e with a per-row exponent spread.  The budget is derived, not measured (see BOUND below).
  c. sentinels, guard zones and finiteness on the ragged cases, for every combination of accumulate and a_colsum.
  d. no state in the named workspace: NaN-filled, holding another shape's partial tiles, twice in a row -- bit-identical.
  e. VIPANT_TN_SPLIT = 2 and 4 (read by the library on every call): a and b under the restated plan's new `splits`.
  f. the pair launch: a and b, and each C bit-identical to the single launch of its problem in the exact sweep.
  g. e4m3: fp64 product of the dequantised operands under the budget of tests/test_fp8_gpu.py (the instruction's adder keeps fewer
     bits than fp32: no exactness), with c and d.

BOUND.  The products of two bf16 numbers are exact in fp32, so all error comes from additions, and an element's error is at most
depth x u x sum of the magnitudes of its terms, where depth is the longest chain of additions one term passes through and u the
relative error of one addition: 2^-23 rather than 2^-24, because the matrix unit's adder may truncate (observed on the e4m3
instruction).  Depth of C[p, q], read from tn_pp_body, tn_reduce_blocks and the host code:
    32          the 32 products of one v_mfma_f32_16x16x32_bf16 (one k-step), however the unit orders them
  + 2 per       the accumulator takes one k-step's sum per MFMA; a workgroup runs `per` K-tiles of two k-steps
  + splits      tn_reduce_blocks adds the `splits` partial tiles one after the other
  + 1           accumulate: the sum is added to what C held (|C0| joins the magnitudes)
against (|A|^T |B|)[p, q].  Depth of a_colsum[p], from the column-sum code of tn_pp_body and colsum_reduce_block:
    4 ceil(per / ntq)    a thread adds 4 rows of each K-tile on which its workgroup has the turn (kt % ntq == tq)
  + 16                   the 16 row groups of a workgroup
  + ceil(parts / 8) + 1  a reduce thread takes every fourth partial into two alternating accumulators
  + 1 + 2                the two accumulators, then the four threads of a column
  + 1                    accumulate
against sum |a|.  The worst error / bound ratio of every case is printed, and written to the file VIPANT_TN_PARITY_LOG names if it is
set (profiles/tn_parity_observed.txt is one such run), so that a later change can tighten the bound with evidence.

Nothing of gemm_tn.hip is out of scope: the file holds the three ping-pong kernels and the reductions these tests reach (the round-1
two-stage kernel that VIPANT_SW_TWO_STAGE used to select was removed), and the plan they follow is csrc/tn_plan.h."""
import os

import pytest
import torch

import tn_plan as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = -54321.0
GUARD = 64               # sentinel rows around C, sentinel elements around a_colsum
WS_GUARD = 4096          # bytes on either side of the workspace
U = 2.0 ** -23
OBSERVED = []


@pytest.fixture(scope="module")
def ops():
    from vipant_amd import _ffi, ops as O
    _ffi.call("vipant_device_check")
    yield O
    path = os.environ.get("VIPANT_TN_PARITY_LOG")
    if OBSERVED and path:
        with open(path, "w") as f:
            f.write("# worst error / bound per case (tests/test_gemm_tn_gpu.py); C and column sums, without | with accumulate\n")
            f.write("".join(line + "\n" for line in OBSERVED))


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def seed_of(case, salt=0):
    M, P, Q = case[:3]
    return (M * 1000003 + P * 1009 + Q) * 8 + salt


def layout(P, Q, lay, unit=8):
    """(lda, ldb, ldc, column offsets of A, B, C) of a layout tag (tests/tn_plan.py); `unit`: what lda and ldb must be multiples of."""
    up = lambda n: T.ceil_div(n, unit) * unit
    if lay == "t":
        return up(P), up(Q), Q, 0, 0, 0
    oa, ob, oc = (3 * unit, unit, 12) if lay == "o" else (0, 0, 0)
    return oa + up(P) + unit, ob + up(Q) + 2 * unit, oc + Q + 4, oa, ob, oc


def place(data, ld, off, poison=NAN, extra_rows=72):
    """`data` as a view into a parent of row length `ld` whose other elements -- `extra_rows` rows at and beyond M (more than a K-tile),
    the columns in front of `off` and behind the data -- are `poison`."""
    M, N = data.shape
    parent = torch.full((M + extra_rows, ld), poison, dtype=data.dtype, device=DEV)
    view = parent[:M, off:off + N]
    view.copy_(data)
    return view


class Out:
    """C [P, Q] and a_colsum [P] as views into sentinel-filled parents."""

    def __init__(self, P, Q, ldc, oc, c0=None, cs0=None):
        self.box = (slice(GUARD, GUARD + P), slice(oc, oc + Q))
        self.c_parent = torch.full((P + 2 * GUARD, ldc), SENTINEL, device=DEV)
        self.cs_parent = torch.full((P + 2 * GUARD,), SENTINEL, device=DEV)
        self.c, self.cs = self.c_parent[self.box], self.cs_parent[GUARD:GUARD + P]
        if c0 is not None:
            self.c.copy_(c0)
        if cs0 is not None:
            self.cs.copy_(cs0)

    def check(self, what, with_cs):
        c, cs = self.c_parent.clone(), self.cs_parent.clone()
        c[self.box] = SENTINEL
        assert bool((c == SENTINEL).all()), f"{what}: written around C[:P, :Q]"
        if with_cs:
            cs[GUARD:-GUARD] = SENTINEL
        assert bool((cs == SENTINEL).all()), f"{what}: written around a_colsum[:P]" if with_cs else f"{what}: a_colsum written without being asked"
        assert bool(torch.isfinite(self.c).all()) and (not with_cs or bool(torch.isfinite(self.cs).all())), f"{what}: not finite"


class Workspace:
    """Exactly `nbytes` of NaN between two guard zones."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 2 * WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.buf[WS_GUARD:WS_GUARD + nbytes] = 0xFF
        self.ptr = self.buf.data_ptr() + WS_GUARD

    def check(self, what):
        assert bool((self.buf[:WS_GUARD] == 0xA5).all()) and bool((self.buf[WS_GUARD + self.nbytes:] == 0xA5).all()), \
            f"{what}: written outside the {self.nbytes} bytes the workspace query asked for"


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_tn(ops, a, b, out, accumulate, with_cs, what):
    """One vipant_gemm_tn call on views, the workspace at its exact size; returns the restated plan of the launch."""
    (M, P), Q = a.shape, b.shape[1]
    l = T.plan(M, P, Q, accumulate)
    nbytes = ops.query("vipant_gemm_tn_workspace_bytes", M, P, Q)
    assert nbytes == l.ws_bytes, (nbytes, l)
    ws = Workspace(nbytes)
    ops.call("vipant_gemm_tn", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.c.data_ptr(), out.c.stride(0), M, P, Q,
             int(accumulate), out.cs.data_ptr() if with_cs else None, ws.ptr, nbytes, stream())
    out.check(what, with_cs)
    ws.check(what)
    return l


def run_pair(ops, a0, b0, o0, a1, b1, o1, what):
    (M, P), Q = a0.shape, b0.shape[1]
    l = T.plan_pair(M, P, Q)
    nbytes = ops.query("vipant_gemm_tn_pair_workspace_bytes", M, P, Q)
    assert nbytes == l.ws_bytes, (nbytes, l)
    assert a0.stride(0) == a1.stride(0) and b0.stride(0) == b1.stride(0) and o0.c.stride(0) == o1.c.stride(0)
    ws = Workspace(nbytes)
    ops.call("vipant_gemm_tn_pair", a0.data_ptr(), b0.data_ptr(), o0.c.data_ptr(), a1.data_ptr(), b1.data_ptr(), o1.c.data_ptr(),
             a0.stride(0), b0.stride(0), o0.c.stride(0), M, P, Q, ws.ptr, nbytes, stream())
    o0.check(what + " (first problem)", False)
    o1.check(what + " (second problem)", False)
    ws.check(what)
    return l


# ------------------------------------------------------------------------------------------------------------------- operands
def int_operands(case, salt=0):
    """(A, B) views with integers in -3..3, and the contiguous data they hold."""
    M, P, Q, lay = case
    lda, ldb, _, oa, ob, _ = layout(P, Q, lay)
    g = gen(seed_of(case, salt))
    a = torch.randint(-3, 4, (M, P), generator=g, device=DEV).to(torch.bfloat16)
    b = torch.randint(-3, 4, (M, Q), generator=g, device=DEV).to(torch.bfloat16)
    return place(a, lda, oa), place(b, ldb, ob), a, b


def gauss_data(case, salt=0):
    """N(0, 1) 2^e, e per row in -6..6 (A) and the same exponents in reverse row order (B), as tests/test_fp8_gpu.py spreads them."""
    M, P, Q, _ = case
    g = gen(seed_of(case, salt + 4))
    e = torch.exp2(torch.randint(-6, 7, (M, 1), generator=g, device=DEV).float())
    a = (torch.randn(M, P, generator=g, device=DEV) * e).to(torch.bfloat16)
    b = (torch.randn(M, Q, generator=g, device=DEV) * e.flip(0)).to(torch.bfloat16)
    return a, b


def gauss_operands(case, salt=0):
    M, P, Q, lay = case
    lda, ldb, _, oa, ob, _ = layout(P, Q, lay)
    a, b = gauss_data(case, salt)
    return place(a, lda, oa), place(b, ldb, ob), a, b


def new_out(case, c0=None, cs0=None):
    _, P, Q, lay = case
    _, _, ldc, _, _, oc = layout(P, Q, lay)
    return Out(P, Q, ldc, oc, c0, cs0)


def ratio(got, ref, bound):
    """Worst |got - ref| / bound; inf where a zero bound is missed."""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------------- a, b: bf16
def exact_case(ops, case):
    M, P, Q, _ = case
    av, bv, a, b = int_operands(case)
    ref, cs_ref = a.double().t() @ b.double(), a.double().sum(0)
    assert 9 * M < 2 ** 16
    out = new_out(case)
    run_tn(ops, av, bv, out, False, False, "exact")
    bad = int((out.c.double() != ref).sum())
    assert bad == 0, f"{case}: {bad} of {P * Q} elements of C differ from the integer product"
    out = new_out(case)
    l = run_tn(ops, av, bv, out, False, True, "exact, column sums")
    bad, bad_cs = int((out.c.double() != ref).sum()), int((out.cs.double() != cs_ref).sum())
    assert bad == 0 and bad_cs == 0, f"{case} {l}: {bad} elements of C, {bad_cs} column sums differ (with a_colsum)"
    g = gen(seed_of(case, 1))
    c0 = torch.randint(-50, 51, (P, Q), generator=g, device=DEV).float()
    cs0 = torch.randint(-50, 51, (P,), generator=g, device=DEV).float()
    out = new_out(case, c0, cs0)
    l = run_tn(ops, av, bv, out, True, True, "exact, accumulate")
    bad, bad_cs = int((out.c.double() != ref + c0.double()).sum()), int((out.cs.double() != cs_ref + cs0.double()).sum())
    assert bad == 0 and bad_cs == 0, f"{case} {l}: {bad} elements of C, {bad_cs} column sums differ (accumulate)"
    out = new_out(case, c0)
    run_tn(ops, av, bv, out, True, False, "exact, accumulate without column sums")
    assert torch.equal(out.c.double(), ref + c0.double()), case


def gauss_case(ops, case, tag=""):
    M, P, Q, _ = case
    av, bv, a, b = gauss_operands(case)
    ad, bd = a.double(), b.double()
    ref, mag = ad.t() @ bd, ad.abs().t() @ bd.abs()
    cs_ref, cs_mag = ad.sum(0), ad.abs().sum(0)
    g = gen(seed_of(case, 2))
    c0 = torch.randn(P, Q, generator=g, device=DEV) * float(ref.abs().mean())
    cs0 = torch.randn(P, generator=g, device=DEV) * float(cs_ref.abs().mean())
    rs = []
    for acc in (False, True):
        out = new_out(case, c0 if acc else None, cs0 if acc else None)
        l = run_tn(ops, av, bv, out, acc, True, "gaussian" + (", accumulate" if acc else ""))
        rc = ratio(out.c, ref + c0.double() if acc else ref, T.depth_c(l, acc) * U * (mag + c0.double().abs() if acc else mag))
        rcs = ratio(out.cs, cs_ref + cs0.double() if acc else cs_ref,
                    T.depth_colsum(l, acc) * U * (cs_mag + cs0.double().abs() if acc else cs_mag))
        rs += [rc, rcs]
    line = "gemm_tn%s %-22s splits %2d per %2d depth %3d / %3d: C %.4f | %.4f  colsum %.4f | %.4f" % (
        tag, T.case_id(case), l.splits, l.per, T.depth_c(l, False), T.depth_colsum(l, False), rs[0], rs[2], rs[1], rs[3])
    print(line)
    OBSERVED.append(line)
    assert max(rs) <= 1.0, line


@pytest.mark.parametrize("case", T.BF16_CASES, ids=T.case_id)
def test_exact_sweep(ops, monkeypatch, case):
    """a.  C, the column sums and both under accumulate equal the integer reference bit for bit."""
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    exact_case(ops, case)


@pytest.mark.parametrize("case", T.BF16_CASES, ids=T.case_id)
def test_gaussian_sweep(ops, monkeypatch, case):
    """b.  Inside depth x 2^-23 x the magnitudes (module docstring: BOUND)."""
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    gauss_case(ops, case)


# ------------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("case", T.RAGGED_CASES, ids=T.case_id)
def test_nothing_is_written_outside_the_outputs(ops, monkeypatch, case):
    """c.  Slab stores are whole 256 x 256 tiles whatever P and Q are, the reads run to the tile's edge and into the next K-tile: the
    sentinels around C and a_colsum, the bytes around the workspace and the outputs' finiteness, for every combination of accumulate
    and a_colsum (run_tn checks them after every call)."""
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    M, P, Q, _ = case
    av, bv, a, b = gauss_operands(case, salt=1)
    ad, bd = a.double(), b.double()
    ref, mag = ad.t() @ bd, ad.abs().t() @ bd.abs()
    for acc in (False, True):
        for with_cs in (False, True):
            out = new_out(case, torch.ones(P, Q, device=DEV) if acc else None, torch.ones(P, device=DEV) if acc and with_cs else None)
            l = run_tn(ops, av, bv, out, acc, with_cs, f"{case} accumulate={acc} a_colsum={with_cs}")
            assert ratio(out.c, ref + 1.0 if acc else ref, T.depth_c(l, acc) * U * (mag + 1.0 if acc else mag)) <= 1.0


# ------------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("case", T.STATE_CASES, ids=T.case_id)
def test_workspace_carries_no_state(ops, monkeypatch, case):
    """d.  The named scratch buffer NaN-filled, then holding the partial tiles of another shape, then of the same call: three
    bit-identical results (ops.gemm_tn, as the block backward calls it)."""
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    M, P, Q, _ = case
    other = (704, 776, 520, "o") if case[:3] != (704, 776, 520) else (385, 100, 260, "p")
    av, bv, _, _ = gauss_operands(case, salt=2)
    ov, pv, _, _ = gauss_operands(other, salt=3)
    need = max(ops.query("vipant_gemm_tn_workspace_bytes", *c[:3]) for c in (case, other))
    results = []

    def once():
        out = new_out(case)
        ops.gemm_tn(av, bv, out.c, a_colsum=out.cs, ws_name="tn_parity")
        out.check("named workspace", True)
        results.append((out.c.clone(), out.cs.clone()))

    ops.scratch("tn_parity", need, torch.device(DEV)).fill_(0xFF)
    once()
    o2 = new_out(other)
    ops.gemm_tn((ov.float() * 1000.0).to(torch.bfloat16), pv.contiguous(), o2.c, a_colsum=o2.cs, ws_name="tn_parity")
    once()
    once()
    for c, cs in results[1:]:
        assert torch.equal(c, results[0][0]) and torch.equal(cs, results[0][1]), case


# ------------------------------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("case", T.SPLIT_ENV_CASES, ids=T.case_id)
def test_split_factor_from_the_environment(ops, monkeypatch, case, factor):
    """e.  VIPANT_TN_SPLIT = 2, 4: more and shorter splits (a direct launch becomes a slab launch).  The exact sweep stays exact, the
    Gaussian sweep inside the bound of the restated plan's new `splits`; run_tn ties that plan to the library's byte count."""
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    before = T.plan(*case[:3])
    monkeypatch.setenv("VIPANT_TN_SPLIT", str(factor))
    after = T.plan(*case[:3])
    assert after.splits > before.splits and after.per < before.per and not after.direct
    exact_case(ops, case)
    gauss_case(ops, case, tag=f" VIPANT_TN_SPLIT={factor}")


# ------------------------------------------------------------------------------------------------------------------- f
def pair_operands(case, make):
    M, P, Q, lay = case
    _, _, ldc, _, _, oc = layout(P, Q, lay)
    x = [make(case, salt=0), make(case, salt=16)]
    return x, [Out(P, Q, ldc, oc), Out(P, Q, ldc, oc)]


@pytest.mark.parametrize("case", T.PAIR_CASES, ids=T.case_id)
def test_pair_exact_sweep(ops, monkeypatch, case):
    """f.  Two problems with different integer data in one launch: each C equals its integer product and the single launch of its
    problem, bit for bit."""
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    M, P, Q, _ = case
    x, o = pair_operands(case, int_operands)
    run_pair(ops, x[0][0], x[0][1], o[0], x[1][0], x[1][1], o[1], "pair, exact")
    assert not torch.equal(x[0][2], x[1][2]) and not torch.equal(x[0][3], x[1][3])
    for (av, bv, a, b), out in zip(x, o):
        ref = a.double().t() @ b.double()
        bad = int((out.c.double() != ref).sum())
        assert bad == 0, f"{case}: {bad} of {P * Q} elements differ from the integer product"
        single = new_out(case)
        run_tn(ops, av, bv, single, False, False, "single launch of a pair's problem")
        assert torch.equal(out.c, single.c), case


@pytest.mark.parametrize("case", T.PAIR_CASES, ids=T.case_id)
def test_pair_gaussian_sweep(ops, case):
    """f.  The bound of (b) with the pair's own plan (twice the tile count enters it: half the splits, twice the K-tiles each)."""
    x, o = pair_operands(case, gauss_operands)
    l = run_pair(ops, x[0][0], x[0][1], o[0], x[1][0], x[1][1], o[1], "pair, gaussian")
    rs = []
    for (_, _, a, b), out in zip(x, o):
        ad, bd = a.double(), b.double()
        rs.append(ratio(out.c, ad.t() @ bd, T.depth_c(l, False) * U * (ad.abs().t() @ bd.abs())))
    line = "gemm_tn_pair %-22s splits %2d per %2d depth %3d: C %.4f, %.4f" % (T.case_id(case), l.splits, l.per, T.depth_c(l, False), *rs)
    print(line)
    OBSERVED.append(line)
    assert max(rs) <= 1.0, line


# ------------------------------------------------------------------------------------------------------------------- g
E4M3_NAN = 0x7F


def e4m3_operand(ops, data, ld):
    """bf16 [M, N] -> (view of the e4m3 bytes in a parent of row length ld, block scales laid out for that row length, the dequantised
    fp64 matrix).  Rows at and beyond M and the padding columns hold the format's NaN byte; scale bytes the quantiser does not write
    (token blocks at and beyond M in the last group of 128) hold 0xFF, the scale format's NaN."""
    M, N = data.shape
    full = torch.zeros(M, ld, dtype=torch.bfloat16, device=DEV)
    full[:, :N] = data
    parent = torch.full((M + 136, ld), E4M3_NAN, dtype=torch.uint8, device=DEV)
    scale = torch.full((ops.query("vipant_mx_scale_bytes", M, ld),), 0xFF, dtype=torch.uint8, device=DEV)
    ops.quant_e4m3_mx32(full, q=parent[:M], scale=scale)
    sc = torch.exp2(scale[ops.mx_scale_index(M, ld, DEV)].double() - 127)
    deq = (parent[:M].view(torch.float8_e4m3fn).double().view(M, ld // 32, 32) * sc[:, :, None]).view(M, ld)[:, :N].contiguous()
    parent[:M, N:] = E4M3_NAN
    return parent[:M, :N], scale, deq


def run_tn8(ops, qa, sa, qb, sb, out, accumulate, with_cs, what):
    (M, P), Q = qa.shape, qb.shape[1]
    l = T.plan8(M, P, Q, accumulate)
    nbytes = ops.query("vipant_gemm_tn_e4m3_workspace_bytes", M, P, Q)
    assert nbytes == l.ws_bytes, (nbytes, l)
    ws = Workspace(nbytes)
    ops.call("vipant_gemm_tn_e4m3", qa.data_ptr(), qa.stride(0), sa.data_ptr(), qb.data_ptr(), qb.stride(0), sb.data_ptr(),
             out.c.data_ptr(), out.c.stride(0), M, P, Q, int(accumulate), out.cs.data_ptr() if with_cs else None, ws.ptr, nbytes, stream())
    out.check(what, with_cs)
    ws.check(what)
    return l


@pytest.mark.parametrize("case", T.E4M3_CASES, ids=T.case_id)
def test_e4m3_sweep(ops, monkeypatch, case):
    """g.  Against the fp64 product of the dequantised operands: C within 4e-4 of the result's largest element, the column sums within
    1e-5 of theirs (the budgets of tests/test_fp8_gpu.py), without and with accumulation; sentinels, workspace bounds and finiteness as
    in (c); and three bit-identical results from a NaN-filled workspace, one holding another shape's tiles, and a repeat, as in (d)."""
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    M, P, Q, lay = case
    lda, ldb, ldc, _, _, oc = layout(P, Q, lay, unit=128)
    a, b = gauss_data(case)
    a[:, 64:96] *= 32.0
    qa, sa, da = e4m3_operand(ops, a, lda)
    qb, sb, db = e4m3_operand(ops, b, ldb)
    ref, cs_ref = da.t() @ db, da.sum(0)
    out = Out(P, Q, ldc, oc)
    l = run_tn8(ops, qa, sa, qb, sb, out, False, True, "e4m3")
    err, err_cs = float((out.c.double() - ref).abs().max() / ref.abs().max()), float((out.cs.double() - cs_ref).abs().max() / cs_ref.abs().max())
    g = gen(seed_of(case, 3))
    c0 = torch.randn(P, Q, generator=g, device=DEV) * float(ref.abs().mean())
    cs0 = torch.randn(P, generator=g, device=DEV) * float(cs_ref.abs().mean())
    out2 = Out(P, Q, ldc, oc, c0, cs0)
    run_tn8(ops, qa, sa, qb, sb, out2, True, True, "e4m3, accumulate")
    ref2, cs_ref2 = ref + c0.double(), cs_ref + cs0.double()
    err2, err_cs2 = float((out2.c.double() - ref2).abs().max() / ref2.abs().max()), float((out2.cs.double() - cs_ref2).abs().max() / cs_ref2.abs().max())
    out3 = Out(P, Q, ldc, oc)
    run_tn8(ops, qa, sa, qb, sb, out3, False, False, "e4m3, no column sums")
    line = "gemm_tn_e4m3 %-22s splits %2d per %2d: C %.2e | %.2e of the largest element (budget 4e-4)  colsum %.2e | %.2e (budget 1e-5)" % (
        T.case_id(case), l.splits, l.per, err, err2, err_cs, err_cs2)
    print(line)
    OBSERVED.append(line)
    assert err < 4e-4 and err2 < 4e-4 and err_cs < 1e-5 and err_cs2 < 1e-5, line
    assert torch.equal(out3.c, out.c), "C depends on whether the column sums ride along"
    # (d) on the named workspace
    other = (1700, 2048, 2048, "p") if case[:3] != (1700, 2048, 2048) else (768, 2304, 2560, "p")
    need = max(ops.query("vipant_gemm_tn_e4m3_workspace_bytes", *c[:3]) for c in (case, other))
    ops.scratch("tn_parity8", need, torch.device(DEV)).fill_(0xFF)
    results = []
    for step in range(3):
        o = Out(P, Q, ldc, oc)
        ops.gemm_tn_e4m3(qa, sa, qb, sb, o.c, a_colsum=o.cs, ws_name="tn_parity8")
        o.check("e4m3, named workspace", True)
        results.append(o)
        if step == 0:
            xa, xb = gauss_data(other, salt=1)
            (xq, xs), (yq, ys) = ops.quant_e4m3_mx32(xa), ops.quant_e4m3_mx32(xb)
            ops.gemm_tn_e4m3(xq, xs, yq, ys, torch.empty(other[1], other[2], device=DEV), ws_name="tn_parity8")
    for o in results:
        assert torch.equal(o.c, out.c) and torch.equal(o.cs, out.cs), case
