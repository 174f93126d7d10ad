"""vipant_infonce_multi_fwd_bwd on the MI355X: several weighted InfoNCE terms over shared operands, against an fp64 restatement.

Every call goes through the C ABI directly: the operands sit inside NaN-poisoned buffers, every output inside a buffer of
sentinels (rows before and after it are checked afterwards), and the workspace has exactly the size the query returns and is
filled with 0xFF bytes (NaN patterns) before every call.

Bounds.  loss[k]: 5e-5 x loss of fp64, the bound the single-pair kernel is documented to hold (tests/test_kernels_gpu.py); the
weighted total: the same on sum_k |w_k| loss_k.  Gradients, each on its own scale (relative L2, and max-abs over the largest
reference entry): 1.5 x the error of an emulation that rounds s.w.dZ and the other operand to bf16 and accumulates in fp64, + 1e-3;
the emulation's error is computed per case.  dlogit_scale: 1e-4 + 1e-3 |ref|, what test_infonce_golden asks of the single-pair
call (it is formed from the fp32-grade log-sum-exp triples, not from bf16 operands), and exactly 0 where the clamp is active.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 777.0
WEIGHTS = (1.0, 0.5, 2.0, 0.25, 1.5)
SCALES = (2.0, 2.6593, 3.1, 2.3, 2.9)
# operands: 0 = prime image features (no gradient), 1 = image view 1, 2 = audio view 1, 3 = image view 2, 4 = audio view 2
GRAPHS = {
    "default": (4, [(1, 0), (1, 2), (1, 3)], (0,)),                          # vp, va, vv of ce_va.yaml
    "full": (5, [(1, 0), (2, 0), (1, 2), (1, 3), (2, 4)], (0,)),             # vp, ap, va, vv, aa
    "apart": (4, [(0, 1), (2, 3)], ()),                                      # two pairs that share nothing
    "one": (2, [(0, 1)], ()),
    "two": (3, [(0, 1), (2, 1)], ()),
    "four": (4, [(0, 1), (1, 2), (2, 3), (3, 0)], (3,)),
    "bare": (4, [(1, 0), (1, 2), (1, 3)], (0, 1, 3)),                        # a frozen image tower: vp and vv have no operand with a gradient
}


@pytest.fixture(scope="module")
def ffi():
    from vipant_amd import _ffi
    _ffi.call("vipant_device_check")
    return _ffi


def operands(B, E, nop, seed=0):
    """nop weakly correlated unit-norm matrices (cosine of matching rows ~ 0.1, as between towers early in training), each a view
    into a NaN-poisoned buffer (one row of NaN before and after).  The correlation is kept weak on purpose: the loss is
    log-sum-exp minus the diagonal logit, two numbers of size s = exp(logit_scale) <= 22 here, so ANY fp32 evaluation carries an
    absolute error of a few 2^-24 s ~ 1e-6, and the relative bound of 5e-5 can only be asked where the loss itself is not driven
    towards 0 by near-identical operands (at B = 2 with cosine 0.6 the fp64 loss is 5e-3 and fp32 rounding alone is 7e-5 of it)."""
    g = torch.Generator(device="cpu"); g.manual_seed(1000 * B + E + seed)
    base = torch.randn(B, E, generator=g)
    out = []
    for _ in range(nop):
        x = base + 3.0 * torch.randn(B, E, generator=g)
        x = x / x.norm(dim=-1, keepdim=True)
        buf = torch.full(((B + 2) * E,), float("nan"), device=DEV)
        buf[E:(B + 1) * E] = x.to(DEV).reshape(-1)
        out.append(buf[E:(B + 1) * E].view(B, E))
    return out


def guarded(rows, cols):
    """A [rows, cols] output inside sentinels; returns (buffer, view)."""
    buf = torch.full(((rows + 2) * cols,), SENTINEL, device=DEV)
    return buf, buf[cols:(rows + 1) * cols].view(rows, cols)


def guards_intact(buf, rows, cols):
    return bool((buf[:cols] == SENTINEL).all()) and bool((buf[(rows + 1) * cols:] == SENTINEL).all())


def call_multi(ffi, xs, pairs, ls, smax, wts, gs, row0, nrows, no_grad=(), forward_only=False):
    """One call; returns dict(loss [npair + 1], dx list (None where not asked), dls) and asserts every guard."""
    nop, npair = len(xs), len(pairs)
    B, E = xs[0].shape
    nbytes = ffi.query("vipant_infonce_multi_workspace_bytes", B, E, nop, npair, 0 if forward_only else nrows)
    assert nbytes > 0
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)           # exact size, dirty
    lbuf, loss = guarded(1, npair + 1)
    dbuf, dls = guarded(1, npair)
    outs = [None if (forward_only or i in no_grad) else guarded(max(nrows, 1), E) for i in range(nop)]
    lsd = torch.tensor(ls, dtype=torch.float32, device=DEV)
    dxtab = None if forward_only else (C.c_void_p * nop)(*[None if o is None else o[1].data_ptr() for o in outs])
    ffi.call("vipant_infonce_multi_fwd_bwd", (C.c_void_p * nop)(*[x.data_ptr() for x in xs]), nop,
             (C.c_int32 * npair)(*[a for a, _ in pairs]), (C.c_int32 * npair)(*[b for _, b in pairs]), npair, lsd.data_ptr(),
             (C.c_float * npair)(*smax), (C.c_float * npair)(*wts), loss.data_ptr(), dxtab, None if forward_only else dls.data_ptr(),
             gs, B, E, row0, nrows, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert guards_intact(lbuf, 1, npair + 1), "loss guards"
    assert guards_intact(dbuf, 1, npair), "dlogit_scale guards"
    if forward_only:
        assert bool((dls == SENTINEL).all())
    dx = []
    for o in outs:
        if o is None:
            dx.append(None)
            continue
        assert guards_intact(o[0], max(nrows, 1), E), "dx guards"
        if nrows == 0:
            assert bool((o[1] == SENTINEL).all())
        dx.append(o[1][:nrows].clone())
    return dict(loss=loss.reshape(-1).clone(), dx=dx, dls=None if forward_only else dls.reshape(-1).clone())


def call_single(ffi, x1, x2, ls, smax, gs, row0, nrows):
    B, E = x1.shape
    nbytes = ffi.query("vipant_infonce_strip_workspace_bytes", B, E, nrows)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    loss = torch.empty(1, device=DEV); dls = torch.empty(1, device=DEV)
    d1 = torch.empty(nrows, E, device=DEV); d2 = torch.empty(nrows, E, device=DEV)
    lsd = torch.tensor([ls], dtype=torch.float32, device=DEV)
    ffi.call("vipant_infonce_fwd_bwd", x1.data_ptr(), x2.data_ptr(), lsd.data_ptr(), smax, loss.data_ptr(), d1.data_ptr(), d2.data_ptr(),
             dls.data_ptr(), gs, B, E, row0, nrows, ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return loss, d1, d2, dls


def bf16_round(t):
    return t.float().to(torch.bfloat16).double()


def reference(xs, pairs, ls, smax, wts, gs):
    """fp64: per-pair losses, total, d total / d x_i * gs, d (w_k loss_k) / d ls_k * gs -- and the bf16-operand emulation of the
    feature gradients (s.w.dZ and the other operand rounded to bf16, fp64 accumulation)."""
    X = [x.double() for x in xs]
    B = X[0].shape[0]
    eye = torch.eye(B, dtype=torch.float64, device=DEV)
    losses, dls = [], []
    dx = [torch.zeros_like(x) for x in X]
    emu = [torch.zeros_like(x) for x in X]
    for k, (a, b) in enumerate(pairs):
        raw = math.exp(ls[k])
        clamped = smax[k] > 0 and raw > smax[k]
        s = smax[k] if clamped else raw
        Z = s * X[a] @ X[b].t()
        lr, lc = torch.logsumexp(Z, 1), torch.logsumexp(Z, 0)
        d = Z.diagonal()
        losses.append(float((lr - d).mean() + (lc - d).mean()))
        dZ = (torch.exp(Z - lr[:, None]) + torch.exp(Z - lc[None, :]) - 2 * eye) / B
        dls.append(0.0 if clamped else float((dZ * Z).sum()) * wts[k] * gs)
        G = gs * wts[k] * s * dZ
        dx[a] += G @ X[b]; dx[b] += G.t() @ X[a]
        Gr = bf16_round(G)
        emu[a] += Gr @ bf16_round(X[b]); emu[b] += Gr.t() @ bf16_round(X[a])
    total = sum(w * l for w, l in zip(wts, losses))
    return losses, total, dx, emu, dls


def errs(got, ref):
    got, ref = got.double(), ref.double()
    return float((got - ref).norm() / ref.norm()), float((got - ref).abs().max() / ref.abs().max())


def check_case(ffi, B, E, graph, row0=0, nrows=None, gs=1.0):
    nop, pairs, no_grad = GRAPHS[graph]
    npair = len(pairs)
    nrows = B if nrows is None else nrows
    xs = operands(B, E, nop)
    ls, wts = list(SCALES[:npair]), list(WEIGHTS[:npair])
    smax = [0.0] * npair
    if npair > 1:
        smax[1] = 10.0            # below exp(2.6593) = 14.29: the clamp is active on exactly one pair
    got = call_multi(ffi, xs, pairs, ls, smax, wts, gs, row0, nrows, no_grad=no_grad)
    losses, total, dx, emu, dls = reference(xs, pairs, ls, smax, wts, gs)
    for k in range(npair):
        print(f"[multi B={B} E={E} {graph}] loss[{k}] hip={float(got['loss'][k]):.7f} fp64={losses[k]:.7f}")
        assert abs(float(got["loss"][k]) - losses[k]) <= 5e-5 * losses[k], (k, float(got["loss"][k]), losses[k])
        print(f"    dls[{k}] hip={float(got['dls'][k]):.6e} fp64={dls[k]:.6e}")
        if smax[k] > 0:
            assert float(got["dls"][k]) == 0.0
        else:
            assert abs(float(got["dls"][k]) - dls[k]) <= 1e-4 + 1e-3 * abs(dls[k]), (k, float(got["dls"][k]), dls[k])
    assert abs(float(got["loss"][npair]) - total) <= 5e-5 * sum(abs(w) * l for w, l in zip(wts, losses)), (float(got["loss"][npair]), total)
    sl = slice(row0, row0 + nrows)
    for i in range(nop):
        if i in no_grad:
            assert got["dx"][i] is None
            continue
        if nrows == 0:
            continue
        assert torch.isfinite(got["dx"][i]).all(), i
        (hl2, hmx), (el2, emx) = errs(got["dx"][i], dx[i][sl]), errs(emu[i][sl], dx[i][sl])
        print(f"    dx[{i}] rel L2 hip={hl2:.3e} emu={el2:.3e}; max-abs hip={hmx:.3e} emu={emx:.3e}")
        assert hl2 <= 1.5 * el2 + 1e-3 and hmx <= 1.5 * emx + 1e-3, (i, hl2, el2, hmx, emx)
    return xs, pairs, ls, smax, wts, got


@pytest.mark.parametrize("B", [2, 7, 16, 17, 130, 432, 768])
def test_fused_default_graph(ffi, B):
    check_case(ffi, B, 512, "default")


@pytest.mark.parametrize("B,graph", [(17, "full"), (130, "full"), (432, "full"), (130, "apart"), (130, "one"), (130, "two"), (130, "four"),
                                     (7, "four")])
def test_fused_graphs(ffi, B, graph):
    check_case(ffi, B, 512, graph, gs=2.0)


@pytest.mark.parametrize("B,E,graph", [(769, 512, "default"), (130, 256, "full"), (130, 256, "apart")])
def test_sequential_path(ffi, B, E, graph):
    check_case(ffi, B, E, graph, gs=2.0)


@pytest.mark.parametrize("B,E,row0,nrows", [(130, 512, 37, 54), (130, 512, 0, 0), (769, 512, 37, 54), (130, 256, 37, 54), (769, 512, 0, 0)])
def test_row_strips_off_the_16_row_grid(ffi, B, E, row0, nrows):
    check_case(ffi, B, E, "full" if B == 130 else "default", row0=row0, nrows=nrows)


@pytest.mark.parametrize("B,E,row0,nrows", [(769, 512, 37, 54), (864, 512, 432, 432), (769, 512, 0, 769), (130, 256, 37, 54), (130, 512, 37, 54)])
def test_pairs_without_a_gradient_operand(ffi, B, E, row0, nrows):
    """ce_va under a frozen image tower: only the audio view asks for a gradient, so two of the three pairs produce none.  On the
    sequential path such a pair takes the single-pair call's full form beside the strip form of the others; the ONE workspace
    query must cover both (B = 864 / 432 rows: two replicas at the default batch)."""
    check_case(ffi, B, E, "bare", row0=row0, nrows=nrows)


@pytest.mark.parametrize("B,E", [(130, 512), (769, 512)])
def test_forward_only(ffi, B, E):
    nop, pairs, _ = GRAPHS["default"]
    xs = operands(B, E, nop)
    ls, wts, smax = list(SCALES[:3]), list(WEIGHTS[:3]), [0.0, 10.0, 0.0]
    got = call_multi(ffi, xs, pairs, ls, smax, wts, 1.0, 0, B, forward_only=True)
    losses, total, *_ = reference(xs, pairs, ls, smax, wts, 1.0)
    for k in range(3):
        assert abs(float(got["loss"][k]) - losses[k]) <= 5e-5 * losses[k]
    assert abs(float(got["loss"][3]) - total) <= 5e-5 * sum(w * l for w, l in zip(wts, losses))


@pytest.mark.parametrize("B,E,row0,nrows", [(17, 512, 0, 17), (130, 512, 0, 130), (432, 512, 108, 108), (130, 512, 37, 54),
                                            (769, 512, 0, 769), (769, 512, 37, 54), (130, 256, 0, 130)])
def test_one_pair_of_weight_one_is_the_single_pair_call(ffi, B, E, row0, nrows):
    """Bit for bit, on the fused path and on the sequential one, clamp off and on."""
    xs = operands(B, E, 2)
    for smax in (0.0, 10.0):
        got = call_multi(ffi, xs, [(0, 1)], [2.6593], [smax], [1.0], 2.0, row0, nrows)
        loss, d1, d2, dls = call_single(ffi, xs[0], xs[1], 2.6593, smax, 2.0, row0, nrows)
        assert torch.equal(got["loss"][0:1], loss) and torch.equal(got["loss"][1:2], loss)
        assert torch.equal(got["dx"][0], d1) and torch.equal(got["dx"][1], d2)
        assert torch.equal(got["dls"], dls)


@pytest.mark.parametrize("B,E", [(130, 512), (432, 512), (769, 512)])
def test_operand_of_one_weight_one_pair_gets_its_single_pair_gradient(ffi, B, E):
    """Default graph, weights 1: the audio view (pair va only) and the second image view (vv only) carry the gradients of the
    single-pair calls bit for bit, every loss[k] is the single-pair loss, and a second call repeats the first exactly."""
    nop, pairs, no_grad = GRAPHS["default"]
    xs = operands(B, E, nop)
    ls = list(SCALES[:3])
    got = call_multi(ffi, xs, pairs, ls, [0.0] * 3, [1.0] * 3, 1.0, 0, B, no_grad=no_grad)
    again = call_multi(ffi, xs, pairs, ls, [0.0] * 3, [1.0] * 3, 1.0, 0, B, no_grad=no_grad)
    assert torch.equal(got["loss"], again["loss"]) and torch.equal(got["dls"], again["dls"])
    for i in (1, 2, 3):
        assert torch.equal(got["dx"][i], again["dx"][i]), i
    for k, (a, b) in enumerate(pairs):
        loss, d1, d2, dls = call_single(ffi, xs[a], xs[b], ls[k], 0.0, 1.0, 0, B)
        assert torch.equal(got["loss"][k:k + 1], loss), k
        assert torch.equal(got["dls"][k:k + 1], dls), k
        if b in (2, 3):
            assert torch.equal(got["dx"][b], d2), k


def test_second_call_repeats_the_first_with_shared_operands(ffi):
    xs, pairs, ls, smax, wts, got = check_case(ffi, 130, 512, "full", gs=2.0)
    again = call_multi(ffi, xs, pairs, ls, smax, wts, 2.0, 0, 130, no_grad=GRAPHS["full"][2])
    assert torch.equal(got["loss"], again["loss"]) and torch.equal(got["dls"], again["dls"])
    for a, b in zip(got["dx"], again["dx"]):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("what", ["gradient for an operand in no pair", "index out of range", "pair with itself", "E % 64", "six pairs"])
def test_refusals_write_nothing(ffi, what):
    B, E = 16, 512
    xs = operands(B, E, 3)
    pairs, nop, Ecall = [(0, 1)], 3, E
    if what == "index out of range":
        pairs = [(0, 3)]
    elif what == "pair with itself":
        pairs = [(1, 1)]
    elif what == "E % 64":
        Ecall = 480
    elif what == "six pairs":
        pairs = [(0, 1)] * 6
    npair = len(pairs)
    lbuf, loss = guarded(1, npair + 1)
    dbuf, dls = guarded(1, npair)
    outs = [guarded(B, E) for _ in range(nop)]          # operand 2 is in no pair and asks for a gradient
    if what != "gradient for an operand in no pair":
        outs[2] = None
    ws = torch.full((1 << 22,), 0xFF, dtype=torch.uint8, device=DEV)
    lsd = torch.full((npair,), 2.0, device=DEV)
    with pytest.raises(ffi.VipantError, match="code -1"):
        ffi.call("vipant_infonce_multi_fwd_bwd", (C.c_void_p * nop)(*[x.data_ptr() for x in xs]), nop,
                 (C.c_int32 * npair)(*[a for a, _ in pairs]), (C.c_int32 * npair)(*[b for _, b in pairs]), npair, lsd.data_ptr(),
                 (C.c_float * npair)(*[0.0] * npair), (C.c_float * npair)(*[1.0] * npair), loss.data_ptr(),
                 (C.c_void_p * nop)(*[None if o is None else o[1].data_ptr() for o in outs]), dls.data_ptr(), 1.0, B, Ecall, 0, B,
                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((lbuf == SENTINEL).all()) and bool((dbuf == SENTINEL).all())
    for o in outs:
        assert o is None or bool((o[0] == SENTINEL).all())
    assert bool((ws == 0xFF).all())
