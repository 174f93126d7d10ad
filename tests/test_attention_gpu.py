"""Attention parity across every kernel instance `dispatch()` (vipant_amd/csrc/attention.hip) can select.

`vipant_mha_fwd` / `vipant_mha_bwd` pick a template instance from S, the causal flag and an edge mode.  `select()` below restates
that choice (seven bucket bounds, the tight / wide edge rule, the 4 / 8 wave backward, the single-pass backward) and
`check_coverage()` asserts -- on the CPU, at import and from tests/test_attention_sweep_cpu.py -- that the sweep's parameter list
reaches every row of this table with both causal values, at both ends of the row's range and at a whole-tile length inside it:

    S          key tiles NT  mask code (EDGE)       forward            backward, non-causal         backward, causal
    1..32           2        last two tiles (= all) mha_fwd_kernel 4w  dQ + dK|dV kernels, 4 waves  dQ + dK|dV, 4 waves
    33..64          4        last two               "                  4 waves                      4 waves
    65..96          6        last two               "                  4 waves                      4 waves
    97..128        10        every tile (EDGE = NT) "                  8 waves                      8 waves
    129..160       10        last two               "                  8 waves                      8 waves
    161..192       14        every tile             "                  8 waves                      8 waves
    193..224       14        last two               "                  8 waves                      8 waves
    225..288       20        every tile             "                  mha_bwd1s_kernel             8 waves
    289..320       20        last two               "                  mha_bwd1s_kernel             8 waves
    321..352       24        every tile             "                  8 waves                      8 waves
    353..384       24        last two               "                  8 waves                      8 waves
    385..          streaming kernels, 64-row chunks, online softmax (forward, dQ, dK|dV), causal and not

(the causal kernels mask in every tile whatever EDGE is; EDGE still selects a different instantiation).

Error metric.  `out`, dQ, dK and dV are judged each on its own scale against an fp64 evaluation (`ref_attention` + autograd) of
the same bf16 inputs: relative L2 error, and largest absolute error relative to the block's own largest value.  The budgets are
not fixed numbers: every case also evaluates `emulate()`, fp64 arithmetic with values rounded to bf16 exactly where the kernels
feed an MFMA or store, and the kernel may have 1.5 x the emulation's error + 1e-3 of the block's scale (the rule of
tests/test_barlow_gpu.py and tests/test_cls_gpu.py).  The roundings, read off attention.hip:

    forward    P~ = bf16(exp(s - m)) before P~ . V, NOT normalised (the row sum l is taken from the unrounded exponentials);
               resident kernels: m = the row's maximum; streaming kernels: m = the running maximum after each 64-key chunk, the
               accumulated P~ . V and l rescaled by exp(m_old - m_new) in fp32;  out = bf16(P~ V / l);  lse = m + log l in fp32
    backward   delta = rowsum(dO * out) from the bf16 `out`;  P = exp(s - lse), bf16 before P^T . dO;
               dS = P * (dP - delta), bf16 before dS . K and dS^T . Q;  dQ, dK = bf16(dS-products / 8), dV = bf16(P^T dO)

`lse` keeps test_mha's 1e-4 relative + 1e-3 absolute.  At S = 1 the exact dQ and dK are zero and "the block's scale" is zero with
them; there the kernel's values are held to the fp32 rounding of dP - delta instead (see `zero_block_bound`).
Every check prints `RATIO <instance> <block> <kernel error> <emulation error>`; DESIGN.md section 5 holds the worst ratios seen.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vipant_amd import _ffi, ops as O
    _ffi.call("vipant_device_check")
    return O


DEV = "cuda:0"


def rnd_cpu(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rnd(*shape, scale=1.0, seed=0, dtype=torch.float32):
    return rnd_cpu(*shape, scale=scale, seed=seed).to(DEV).to(dtype)


def ref_attention(qkv, batch, S, H, causal):
    D = H * 64
    q, k, v = qkv.double().view(batch, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s + torch.full((S, S), float("-inf"), device=s.device, dtype=s.dtype).triu_(1)
    p = torch.softmax(s, -1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(batch * S, D)
    return o, torch.logsumexp(s, -1)


# ------------------------------------------------------------------------------- which instance runs (restates dispatch())
NT_BUCKETS = (2, 4, 6, 10, 14, 20, 24)          # VIPANT_MHA_CASE(NT): S <= 16 NT, first match; beyond the last: streaming
STREAM_CHUNK = 64


def select(S, causal):
    """(NT, EDGE, causal, backward kind) of the instance dispatch() launches; NT = EDGE = 0 for the streaming kernels."""
    for nt in NT_BUCKETS:
        if S <= 16 * nt:
            tight = S > (nt - 2) * 16                                  # launch_fwd / launch_bwd
            edge = min(nt, 2) if tight else nt
            if nt == 20 and not causal:
                bwd = "bwd1s"                                          # persistent single pass, both edge ranges
            else:
                bwd = "2pass-8w" if nt >= 8 else "2pass-4w"
            return nt, edge, bool(causal), bwd
    return 0, 0, bool(causal), "stream"


def instance_name(S, causal):
    nt, edge, c, bwd = select(S, causal)
    return f"{'stream' if nt == 0 else f'NT{nt}/EDGE{edge}'}/{'causal' if c else 'full'}/{bwd}"


def instance_rows():
    """Every (NT, EDGE) row of the table with its range of S, from the seven bounds."""
    rows, prev = [], 0
    for nt in NT_BUCKETS:
        lo, hi, split = prev + 1, 16 * nt, (nt - 2) * 16
        if split >= lo:
            rows.append((nt, nt, lo, split))
        rows.append((nt, min(nt, 2), max(lo, split + 1), hi))
        prev = hi
    return rows


RESIDENT_S = (1, 2, 15, 16, 17, 32, 33, 48, 64, 65, 80, 96, 97, 112, 128, 129, 144, 160, 161, 176, 192, 193, 208, 224, 225, 256,
              288, 289, 304, 320, 321, 336, 352, 353, 368, 384)
STREAM_S = (385, 448, 449, 512)
SWEEP = [(S, c) for S in RESIDENT_S + STREAM_S for c in (False, True)]


def check_coverage(cases):
    """Every row of the table, causal and not: the row's first and last S and a whole number of tiles strictly inside it; the single
    pass backward in both of its rows; the streaming kernels at their first S, at whole chunks and at one row in the last chunk."""
    have = set(cases)
    assert {nt for nt, _, _, _ in instance_rows()} == set(NT_BUCKETS)
    assert {nt for nt, e, _, _ in instance_rows() if e == nt and nt > 2} == {10, 14, 20, 24}, "the rows with mask code everywhere"
    for causal in (False, True):
        for nt, edge, lo, hi in instance_rows():
            inside = [S for S in range(lo + 1, hi) if S % 16 == 0]
            assert inside, (nt, edge)
            for what, want in (("first", [lo]), ("last", [hi]), ("whole tiles inside", inside)):
                hit = [S for S in want if (S, causal) in have]
                assert hit, f"NT={nt} EDGE={edge} causal={causal}: no case at the {what} length ({want})"
                assert all(select(S, causal)[:3] == (nt, edge, causal) for S in hit), (nt, edge, causal, hit)
        first = 16 * NT_BUCKETS[-1] + 1
        stream = [S for S, c in have if c == causal and S >= first]
        assert all(select(S, causal)[3] == "stream" for S in stream)
        assert first in stream and select(first - 1, causal)[0] == NT_BUCKETS[-1], "the resident -> streaming switch"
        assert any(S % STREAM_CHUNK == 0 for S in stream), "no streaming length of whole chunks"
        assert any(S % STREAM_CHUNK == 1 for S in stream), "no streaming length with one row in the last chunk"
    kinds = {(select(S, c)[3], c) for S, c in have}
    assert kinds == {(k, c) for k in ("2pass-4w", "2pass-8w", "stream") for c in (False, True)} | {("bwd1s", False)}, kinds
    assert {select(S, c)[1] == 2 for S, c in have if select(S, c)[3] == "bwd1s"} == {True, False}, "bwd1s in both edge ranges"


check_coverage(SWEEP)          # at import: a list that lost a row is a collection error, with or without a GPU


# ------------------------------------------------------------------------------- bf16-operand emulation
def bf(x):
    return x.to(torch.bfloat16).double()


def split_heads(t, batch, S, H):
    return t.double().view(batch, S, H, 64).permute(0, 2, 1, 3)                  # [batch, H, S, 64]


def merge_heads(t, batch, S, H):
    return t.permute(0, 2, 1, 3).reshape(batch * S, H * 64)


def emulate(qkv, dout, batch, S, H, causal):
    """fp64 with the kernels' bf16 roundings (module docstring): out, lse, dqkv in the kernels' layouts."""
    q, k, v = qkv.double().view(batch, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if causal:
        s = s + torch.full((S, S), float("-inf"), device=s.device, dtype=s.dtype).triu_(1)
    if select(S, causal)[3] != "stream":
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        o = bf(e) @ v
    else:
        m = torch.full_like(s[..., :1], float("-inf"))
        l = torch.zeros_like(m)
        o = torch.zeros_like(q)
        for c in range(0, S, STREAM_CHUNK):
            sc = s[..., c:c + STREAM_CHUNK]
            mn = torch.maximum(m, sc.amax(-1, keepdim=True))                    # finite from chunk 0 on: key 0 is never masked
            alpha = torch.exp(m - mn)
            e = torch.exp(sc - mn)
            l = l * alpha + e.sum(-1, keepdim=True)
            o = o * alpha + bf(e) @ v[..., c:c + STREAM_CHUNK, :]
            m = mn
    ob = bf(o / l)
    lse = (m + torch.log(l)).float().double()
    do = split_heads(dout, batch, S, H)
    delta = (do * ob).sum(-1, keepdim=True)
    p = torch.exp(s - lse)
    ds = bf(p * (do @ v.transpose(-1, -2) - delta))
    dq = bf(0.125 * (ds @ k))
    dk = bf(0.125 * (ds.transpose(-1, -2) @ q))
    dv = bf(bf(p).transpose(-1, -2) @ do)
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(batch * S, 3 * H * 64)
    return merge_heads(ob, batch, S, H), lse.squeeze(-1), dqkv


def zero_block_bound(qkv, dout, batch, S, H):
    """S = 1: P = 1, out = v, so dS = dP - delta = dO.v - dO.v and dQ = dK = 0 exactly.  The kernels take dP on the MFMA and delta
    from a scalar loop, two fp32 sums of the same 64 products in different orders: each is within 64 x 2^-24 x sum|dO_d v_d| of the
    exact value, so |dS| <= 2 x that, and |dQ|, |dK| <= |dS| x max(|k|, |q|) / 8, bf16-rounded twice (dS, the result)."""
    q, k, v = qkv.double().view(batch, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    do = split_heads(dout, batch, S, H)
    ds = 2 * 64 * 2.0 ** -24 * (do.abs() * v.abs()).sum(-1).max()
    return float(ds * max(k.abs().max(), q.abs().max()) * 0.125 * (1 + 2.0 ** -8) ** 2)


def check_block(tag, name, got, emu, ref, zero_bound=None):
    got, emu, ref = got.double(), emu.double(), ref.double()
    assert got.shape == ref.shape == emu.shape, (tag, name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{tag} {name}: non-finite output"
    n, mx = float(ref.norm()), float(ref.abs().max())
    e_hip, e_emu = float((got - ref).norm()), float((emu - ref).norm())
    a_hip, a_emu = float((got - ref).abs().max()), float((emu - ref).abs().max())
    print(f"RATIO {tag} {name} l2 {e_hip / max(n, 1e-300):.3e} {e_emu / max(n, 1e-300):.3e} "
          f"max {a_hip / max(mx, 1e-300):.3e} {a_emu / max(mx, 1e-300):.3e}")
    if zero_bound is not None:
        assert mx <= 1e-12, (tag, name, "the exact block is not zero", mx)
        assert a_hip <= zero_bound, (tag, name, a_hip, zero_bound)
        return
    assert e_hip <= 1.5 * e_emu + 1e-3 * n, (tag, name, "L2: kernel, emulation, block norm", e_hip, e_emu, n)
    assert a_hip <= 1.5 * a_emu + 1e-3 * mx, (tag, name, "max abs: kernel, emulation, block max", a_hip, a_emu, mx)


def check_lse(tag, got, ref):
    got, ref = got.double(), ref.double()
    assert torch.isfinite(got).all(), f"{tag} lse: non-finite"
    bad = (got - ref).abs() > 1e-3 + 1e-4 * ref.abs()
    assert not bad.any(), (tag, "lse", torch.nonzero(bad)[0].tolist(), float((got - ref).abs().max()))


def blocks(dqkv, H):
    d = dqkv.view(dqkv.shape[0], 3, H * 64)
    return {"dQ": d[:, 0], "dK": d[:, 1], "dV": d[:, 2]}


def parity(ops, tag, qkv, dout, batch, S, H, causal):
    """Forward and backward of one problem against fp64 under the metric of the module docstring.  Returns what the tests that look
    at single rows need: the kernel's and the reference's results and the per-block absolute budgets."""
    out, lse = ops.mha_fwd(qkv, batch, S, H, causal)
    dqkv = ops.mha_bwd(qkv, out, dout, lse, batch, S, H, causal)
    qr = qkv.double().requires_grad_()
    ref, rlse = ref_attention(qr, batch, S, H, causal)
    ref.backward(dout.double())
    ref, rgrad = ref.detach(), qr.grad
    e_out, e_lse, e_dqkv = emulate(qkv, dout, batch, S, H, causal)
    check_lse(tag + " emulation", e_lse, rlse)                   # the emulation is the same function
    check_block(tag, "out", out, e_out, ref)
    check_lse(tag, lse, rlse)
    zb = zero_block_bound(qkv, dout, batch, S, H) if S == 1 else None
    gb, eb, rb = blocks(dqkv, H), blocks(e_dqkv, H), blocks(rgrad, H)
    budget = {}
    for name in ("dQ", "dK", "dV"):
        check_block(tag, name, gb[name], eb[name], rb[name], zb if name != "dV" else None)
        budget[name] = 1.5 * float((eb[name] - rb[name]).abs().max()) + 1e-3 * float(rb[name].abs().max())
    return {"out": out, "lse": lse, "dqkv": dqkv, "ref_out": ref, "ref_lse": rlse, "ref_dqkv": rgrad, "budget": budget}


# ------------------------------------------------------------------------------- 1. the sweep
@pytest.mark.parametrize("S,causal", SWEEP, ids=[f"S{S}-{'causal' if c else 'full'}" for S, c in SWEEP])
def test_instance_sweep(ops, S, causal):
    """batch = 2 (the last tile of item 0 lies next to item 1), H = 3 (odd: the bh / H, bh % H paths)."""
    batch, H = 2, 3
    qkv = rnd(batch * S, 3 * H * 64, seed=1, dtype=torch.bfloat16, scale=1.5)
    dout = rnd(batch * S, H * 64, seed=2, dtype=torch.bfloat16)
    parity(ops, instance_name(S, causal), qkv, dout, batch, S, H, causal)


# ------------------------------------------------------------------------------- 3. concentrated softmax rows
SPIKE_AT = (1, 1)                   # (item, head) of batch = 2, H = 2 that carries the constructed rows
# S, causal, query i, dominant keys a and b: different key tiles (different 64-key chunks when streaming), one before and one
# after the query's own block where the mask permits; the same query vector again at S - 2, in the last query block
# (the queries are those, inside these blocks, at which row i of dQ is largest against the rest: 0.016 .. 0.058 of max|dQ|)
SPIKY = [(230, False, 108, 45, 185), (316, False, 158, 40, 290), (352, False, 178, 50, 330), (450, False, 175, 100, 400),
         (1213, False, 544, 70, 1150), (77, True, 58, 10, 40), (200, True, 155, 20, 120), (450, True, 281, 100, 250)]
SPIKY_LEAD = {40: 9.0, 250: 60.0}


def head_view(t, S, width, part=None):
    """[S, 64] view of SPIKE_AT's rows in a packed [2 S, width * 128] tensor (width = 3: part selects q / k / v)."""
    v = t.view(2, S, width, 2, 64)[SPIKE_AT[0], :, :, SPIKE_AT[1]]
    return v[:, 0 if part is None else part]


def spiky_case(S, gain, i, a, b):
    """CPU tensors (qkv, dout) of a batch = 2, H = 2 problem whose head SPIKE_AT has keys a and b dominating queries i and S - 2."""
    qkv = rnd_cpu(2 * S, 384, seed=3, scale=0.2).to(torch.bfloat16)
    q, k = head_view(qkv, S, 3, 0), head_view(qkv, S, 3, 1)
    ka = q[i].float() * gain
    k[a] = ka.to(torch.bfloat16)
    k[b] = (ka + rnd_cpu(64, seed=4)).to(torch.bfloat16)          # exactly equal keys would make the dQ row identically zero
    q[S - 2] = q[i]
    return qkv, rnd_cpu(2 * S, 128, seed=2).to(torch.bfloat16)


def spiky_premises(qkv, dout, S, causal, gain, i, a, b):
    """On the fp64 reference: both dominant probabilities of row i >= 0.2, their lead over every other visible key >= 9 (gain 40) /
    60 (gain 250), and max|dQ[i]| >= 1e-2 max|dQ| (the cancellation in dS = P (dP - delta) is exercised, not trivially zero)."""
    same_tile = (a // 16 == b // 16) or (select(S, causal)[3] == "stream" and a // STREAM_CHUNK == b // STREAM_CHUNK)
    assert not same_tile and len({i, a, b, S - 2}) == 4
    blk = STREAM_CHUNK if select(S, causal)[3] == "stream" else 16
    assert a // blk < i // blk and (b // blk < i // blk if causal else b // blk > i // blk) and (S - 2) // blk == (S - 1) // blk
    qr = qkv.double().requires_grad_()
    ref, _ = ref_attention(qr, 2, S, 2, causal)
    ref.backward(dout.double())
    q, k = head_view(qkv, S, 3, 0).double(), head_view(qkv, S, 3, 1).double()
    s = (q[i] @ k.t()) * 0.125
    if causal:
        s[i + 1:] = float("-inf")
    p = torch.softmax(s, -1)
    others = s.clone(); others[[a, b]] = float("-inf")
    lead = float(torch.minimum(s[a], s[b]) - others.max())
    dq = head_view(qr.grad, S, 3, 0)
    row = float(dq[i].abs().max() / dq.abs().max())
    print(f"spiky S={S} causal={causal} gain={gain}: p[a]={float(p[a]):.3f} p[b]={float(p[b]):.3f} lead={lead:.1f} dQ row {row:.3f}")
    assert float(p[a]) >= 0.2 and float(p[b]) >= 0.2, (float(p[a]), float(p[b]))
    assert lead >= SPIKY_LEAD[gain], lead
    assert row >= 1e-2, row


SPIKY_CASES = [(S, c, g, i, a, b) for S, c, i, a, b in SPIKY for g in (40, 250)]


@pytest.mark.parametrize("S,causal,gain,i,a,b", SPIKY_CASES,
                         ids=[f"S{S}-{'causal' if c else 'full'}-gain{g}" for S, c, g, _, _, _ in SPIKY_CASES])
def test_concentrated_rows(ops, S, causal, gain, i, a, b):
    """Two keys hold a softmax row between them, forward and backward, resident and streaming: the streaming forward has to rescale
    its running maximum when the second key arrives, and every backward meets dS = P (dP - delta) with P near 1/2, where it cancels."""
    qkv, dout = (t.to(DEV) for t in spiky_case(S, gain, i, a, b))
    spiky_premises(qkv, dout, S, causal, gain, i, a, b)
    parity(ops, f"spiky{gain} " + instance_name(S, causal), qkv, dout, 2, S, 2, causal)


# ------------------------------------------------------------------------------- 4. a masked key with a dominant raw score
MASKED = [(77, 20, 60), (200, 50, 150), (352, 100, 300), (450, 120, 400)]       # S, query i (first third), key j > i in a later tile / chunk
MASKED_LEAD = 110.0        # beyond it expf(visible - masked) is zero in fp32, subnormals included: a maximum taken over the masked
                           # score leaves a row sum of 0


def masked_case(S, i, j):
    qkv = rnd_cpu(2 * S, 384, seed=3, scale=0.2).to(torch.bfloat16)
    q, k = head_view(qkv, S, 3, 0), head_view(qkv, S, 3, 1)
    k[j] = (q[i].float() * 600).to(torch.bfloat16)
    return qkv, rnd_cpu(2 * S, 128, seed=2).to(torch.bfloat16)


def masked_premises(qkv, S, i, j):
    blk = STREAM_CHUNK if select(S, True)[3] == "stream" else 16
    assert i < S // 3 and j // blk > i // blk
    q, k = head_view(qkv, S, 3, 0).double(), head_view(qkv, S, 3, 1).double()
    s = (q[i] @ k.t()) * 0.125
    lead = float(s[j] - s[:i + 1].max())
    print(f"masked S={S}: raw score of key {j} for query {i} leads the visible ones by {lead:.1f}")
    assert lead > MASKED_LEAD, lead


@pytest.mark.parametrize("S,i,j", MASKED, ids=[f"S{S}" for S, _, _ in MASKED])
def test_masked_dominant_key(ops, S, i, j):
    """Causal: key j > i scores far above everything query i may see.  Row i must come out as if the key were not there (a maximum
    or a probability taken before the mask gives 0 / 0 or a row that is all key j), and key j's gradients must hold nothing of it."""
    qkv, dout = (t.to(DEV) for t in masked_case(S, i, j))
    masked_premises(qkv, S, i, j)
    r = parity(ops, "masked " + instance_name(S, True), qkv, dout, 2, S, 2, True)
    assert torch.isfinite(r["out"].float()).all() and torch.isfinite(r["lse"]).all()
    assert torch.isfinite(r["dqkv"].float()).all()
    # a leak of row i into key j would add P[i, j] dO[i] ~ dO[i] to dV[j] and P[i, j] (dP - delta) q[i] / 8 to dK[j]
    leak = float(head_view(dout, S, 1)[i].double().abs().max())
    assert leak > 10 * r["budget"]["dV"], (leak, r["budget"]["dV"])
    for name, part in (("dK", 1), ("dV", 2)):
        got, want = head_view(r["dqkv"], S, 3, part)[j].double(), head_view(r["ref_dqkv"], S, 3, part)[j]
        assert float((got - want).abs().max()) <= r["budget"][name], (name, j)


# ------------------------------------------------------------------------------- 5. bounds
# one S per instance family: NT <= 6 (4 waves), NT 10 wide, NT 14 tight, NT 20 wide / tight (bwd1s when not causal), NT 24, streaming
BOUNDS = [(S, c) for S in (31, 126, 200, 230, 316, 370, 428) for c in (False, True)]
BOUNDS_IDS = [f"S{S}-{'causal' if c else 'full'}" for S, c in BOUNDS]
PAD_ROWS = 64
POISON = {torch.bfloat16: (torch.int16, [0x7F80, 0x7FC0, 0x7F62]),                   # +inf, NaN, 3.0e38
          torch.float32: (torch.int32, [0x7F800000, 0x7FC00000, 0x7F61B1E6])}


class Padded:
    """A [rows, cols] tensor inside a larger allocation: PAD_ROWS rows of padding before and after, filled with zeros, with 0xAA
    bytes or with +inf / NaN / 3e38 patterns.  The interior starts as the padding does."""

    def __init__(self, rows, cols, dtype, fill):
        esz = torch.empty((), dtype=dtype).element_size()
        self.pad, n = PAD_ROWS * cols * esz, rows * cols * esz
        assert self.pad % 16 == 0
        self.raw = torch.empty(2 * self.pad + n, dtype=torch.uint8, device=DEV)
        if fill == "poison":
            it, pat = POISON[dtype]
            typed = self.raw.view(it)
            typed.copy_(torch.tensor(pat, dtype=torch.int64).repeat(typed.numel() // len(pat) + 1)[:typed.numel()].to(it))
        else:
            self.raw.fill_({"zero": 0, "aa": 0xAA}[fill])
        self.x = self.raw[self.pad:self.pad + n].view(dtype).view(rows, cols)
        self.before, self.after = self.raw[:self.pad].clone(), self.raw[self.pad + n:].clone()

    def intact(self):
        return torch.equal(self.raw[:self.pad], self.before) and torch.equal(self.raw[-self.pad:], self.after)


def run_padded(ops, qkv, dout, batch, S, H, causal, fill):
    """Forward and backward with every tensor of the two calls placed as a view inside a Padded allocation."""
    M, D = batch * S, H * 64
    t = {"qkv": Padded(M, 3 * D, torch.bfloat16, fill), "out": Padded(M, D, torch.bfloat16, fill),
         "dout": Padded(M, D, torch.bfloat16, fill), "dqkv": Padded(M, 3 * D, torch.bfloat16, fill),
         "lse": Padded(batch * H, S, torch.float32, fill), "delta": Padded(batch * H, S, torch.float32, fill)}
    t["qkv"].x.copy_(qkv); t["dout"].x.copy_(dout)
    p = {k: v.x.data_ptr() for k, v in t.items()}
    st = torch.cuda.current_stream().cuda_stream
    ops.call("vipant_mha_fwd", p["qkv"], p["out"], p["lse"], None, None, batch, S, H, int(causal), st)
    ops.call("vipant_mha_bwd", p["qkv"], p["out"], p["dout"], p["lse"], p["delta"], p["dqkv"], None, None, batch, S, H, int(causal), st)
    torch.cuda.synchronize()
    res = {k: t[k].x.clone() for k in ("out", "lse", "delta", "dqkv")}
    return res, {k: v.intact() for k, v in t.items()}


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def bounds_inputs(batch, S, H):
    return (rnd(batch * S, 3 * H * 64, seed=21, dtype=torch.bfloat16, scale=1.5), rnd(batch * S, H * 64, seed=22, dtype=torch.bfloat16))


@pytest.mark.parametrize("S,causal", BOUNDS, ids=BOUNDS_IDS)
def test_padding_is_not_read(ops, S, causal):
    """(a) what lies before and after the tensors -- allocated memory, so nothing can fault -- does not reach a result: zeros there
    and +inf / NaN / 3e38 there give the same bits.  A partial tile of the last item reads rows past batch * S; a result row the
    kernels fail to write keeps its (different) initial pattern and shows up here as well."""
    batch, H = 3, 2
    qkv, dout = bounds_inputs(batch, S, H)
    zero, _ = run_padded(ops, qkv, dout, batch, S, H, causal, "zero")
    poison, _ = run_padded(ops, qkv, dout, batch, S, H, causal, "poison")
    for k in ("out", "lse", "dqkv"):
        assert torch.isfinite(zero[k].float()).all(), k
        assert same_bits(zero[k], poison[k]), f"{k} depends on memory outside the tensors"


@pytest.mark.parametrize("S,causal", BOUNDS, ids=BOUNDS_IDS)
def test_guard_zones_are_not_written(ops, S, causal):
    """(b) 0xAA bytes on both sides of out, lse, delta and dqkv (and of the inputs) are unchanged after the two calls, and the
    results inside are those of the plain call."""
    batch, H = 3, 2
    qkv, dout = bounds_inputs(batch, S, H)
    res, intact = run_padded(ops, qkv, dout, batch, S, H, causal, "aa")
    assert all(intact.values()), {k: v for k, v in intact.items() if not v}
    out, lse = ops.mha_fwd(qkv, batch, S, H, causal)
    dqkv = ops.mha_bwd(qkv, out, dout, lse, batch, S, H, causal)
    assert same_bits(res["out"], out) and same_bits(res["lse"].view(batch, H, S), lse) and same_bits(res["dqkv"], dqkv)


def alone(ops, qkv, dout, item, S, H, causal):
    """Item `item` of the batch as a batch = 1 problem of its own (fresh tensors: nothing of the neighbours is adjacent)."""
    q1, d1 = qkv[item * S:(item + 1) * S].clone(), dout[item * S:(item + 1) * S].clone()
    out, lse = ops.mha_fwd(q1, 1, S, H, causal)
    return out, lse, ops.mha_bwd(q1, out, d1, lse, 1, S, H, causal)


def check_items(ops, qkv, dout, batch, S, H, causal, items):
    out, lse = ops.mha_fwd(qkv, batch, S, H, causal)
    dqkv = ops.mha_bwd(qkv, out, dout, lse, batch, S, H, causal)
    assert torch.isfinite(dqkv.float()).all()
    for it in items:
        o1, l1, g1 = alone(ops, qkv, dout, it, S, H, causal)
        rows = slice(it * S, (it + 1) * S)
        assert same_bits(out[rows], o1), f"out of item {it}"
        assert same_bits(lse[it], l1[0]), f"lse of item {it}"
        assert same_bits(dqkv[rows], g1), f"dqkv of item {it}"


@pytest.mark.parametrize("S,causal", BOUNDS, ids=BOUNDS_IDS)
def test_items_do_not_leak(ops, S, causal):
    """(c) every item of a batch of 3 has the bits of the batch = 1 call on that item alone: the partial tiles of items 0 and 1 read
    the next item's rows, and none of that may count."""
    batch, H = 3, 2
    qkv, dout = bounds_inputs(batch, S, H)
    check_items(ops, qkv, dout, batch, S, H, causal, range(batch))


def test_persistent_backward_keeps_nothing_between_problems(ops):
    """mha_bwd1s_kernel with batch * H above twice the CU count: every workgroup takes a second and a third problem from the ticket
    walk, reusing its K images, exchange buffers, ring and statistics in LDS.  Items 0, one in the middle and the last must have
    the bits of their batch = 1 calls (one problem per workgroup, fresh LDS)."""
    S, H = 230, 12
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = math.ceil((2 * cus + 1) / H)
    assert batch * H > 2 * cus and select(S, False)[3] == "bwd1s"
    qkv, dout = bounds_inputs(batch, S, H)
    check_items(ops, qkv, dout, batch, S, H, False, (0, batch // 2, batch - 1))
