"""`vipant_resample` / `vipant_resample_table` on the MI355X, through the C ABI, against the DENSE definition in float64 (`dense`: all
2w + o taps of every phase, clamp included -- nothing of the kernel's sparse ranges).  Per pair one ragged launch: Gaussian clips at the
lengths where the kernel changes path (0, 1, T - 1, one workgroup's input span - 1 / exactly / + 1 -- read from the plan --, a length
whose new length is no multiple of n) and unit impulses, which return the table itself.  The input rows are NaN past their length and
both strides are odd, the output lies between NaN guard rows and the lengths between sentinels.
Bound per output: (T + 2) 2^-24 sum_k |K[j,k]| |x_k| + fp32's smallest normal -- one rounding of each coefficient, one per FMA, depth T.
Observed error / bound (MI355X, largest over a pair's outputs): 0.02 ... 0.30 (profiles/resample_observed.txt)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TARGET = {16000: "copy", 48000: "n = 1", 8000: "o = 1", 44100: "n = 160, o = 441", 11025: "n = 640 > 256 threads", 192000: "T = 145"}
# (source, target): the issue's seven; one whose table and span need the LDS opt-in above 64 KB; one whose workgroups own P = 3 periods,
# one per thread, because four do not fit
PAIRS = [(r, 16000) for r in TARGET] + [(16000, 44100), (96000, 11025), (192000, 11025)]
TINY = float(np.finfo(np.float32).tiny)


def dense(orig, new, L=6, rolloff=0.99):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    w = math.ceil(L * o / base)
    j, k = np.arange(n, dtype=np.float64)[:, None], np.arange(2 * w + o, dtype=np.float64)[None, :]
    t = np.clip((-j / n + (k - w) / o) * base, -L, L)
    pt = np.where(t == 0, 1.0, np.pi * t)
    return o, n, w, np.where(t == 0, 1.0, np.sin(pt) / pt) * np.cos(np.pi * t / (2 * L)) ** 2 * base / o


def reference(x, orig, new):
    """-> (out float64 [len_out], sum_k |K| |x| per output)"""
    o, n, w, K = dense(orig, new)
    len_out = -(-n * len(x) // o)
    periods = -(-len_out // n)
    xp = np.concatenate([np.zeros(w), x.astype(np.float64), np.zeros(periods * o + K.shape[1])])
    X = np.lib.stride_tricks.sliding_window_view(xp, K.shape[1])[::o][:periods]
    return (X @ K.T).reshape(-1)[:len_out], (np.abs(X) @ np.abs(K).T).reshape(-1)[:len_out]


@pytest.fixture(scope="module")
def resamplers():
    from vipant_amd.frontend import Resample
    return {16000: Resample(16000, device=DEV), 44100: Resample(44100, device=DEV), 11025: Resample(11025, device=DEV)}


def new_length(resamplers, pair, k):
    plan = resamplers[pair[1]].plan(pair[0])
    return -(-plan.n * k // plan.o)


def launch(resamplers, rows, pairs, out_stride=None):
    """rows: float32 arrays, row i of pair pairs[i] -> (out [b, out_stride], nsamples_out [b]); checks guards, lengths and zeros."""
    from vipant_amd import _ffi
    kinds = sorted(set(pairs))
    classes = (_ffi.ResampleClass * len(kinds))(*[resamplers[new]._class(orig) for orig, new in kinds])
    cls = (C.c_int32 * len(rows))(*[kinds.index(p) for p in pairs])
    b, stride = len(rows), max(len(r) for r in rows) + 5
    want = [new_length(resamplers, p, len(r)) for r, p in zip(rows, pairs)]
    out_stride = out_stride or max(want) + 3
    wave = np.full((b, stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        wave[i, :len(r)] = r
    wave = torch.from_numpy(wave).to(DEV)
    ns = torch.tensor([len(r) for r in rows], dtype=torch.int64, device=DEV)
    out = torch.full((b + 2, out_stride), float("nan"), dtype=torch.float32, device=DEV)
    nout = torch.full((b + 2,), -77, dtype=torch.int64, device=DEV)
    _ffi.call("vipant_resample", wave.data_ptr(), stride, ns.data_ptr(), cls, classes, len(kinds), out[1:].data_ptr(), out_stride,
              nout[1:].data_ptr(), b, None)
    out, nout = out.cpu().numpy(), nout.cpu().numpy()
    assert np.isnan(out[0]).all() and np.isnan(out[-1]).all() and nout[0] == nout[-1] == -77
    out, nout = out[1:-1], nout[1:-1]
    assert nout.tolist() == [min(v, out_stride) for v in want]
    assert all(not out[i, k:].any() and not np.isnan(out[i]).any() for i, k in enumerate(nout))
    return out, nout


@pytest.mark.parametrize("orig,new", PAIRS)
def test_ragged_batch_against_the_dense_definition(resamplers, orig, new):
    plan = resamplers[new].plan(orig)
    o, n, w, K = dense(orig, new)
    if orig != new:
        assert (plan.o, plan.n, plan.w) == (o, n, w) and plan.T == int((np.abs(K).astype(np.float32) > 0).sum(1).max())
    span = plan.P * plan.o                                     # the inputs of one workgroup's P n outputs
    odd = next((k for k in range(o + 1, 3 * o + 3) if (-(-n * k // o)) % n), o + 1)      # (n = 1 or o = 1: there is none)
    lengths = sorted({0, 1, max(plan.T - 1, 0), span - 1, span, span + 1, odd})
    g = np.random.default_rng(orig + new)
    rows = [g.standard_normal(k).astype(np.float32) for k in lengths]
    spikes = max(span + 1, w + 2)
    for pos in (0, w, spikes - 1):
        rows.append(np.zeros(spikes, dtype=np.float32))
        rows[-1][pos] = 1.0
    out, nout = launch(resamplers, rows, [(orig, new)] * len(rows))
    worst = 0.0
    for i, x in enumerate(rows):
        got = out[i, :nout[i]].astype(np.float64)
        if orig == new:
            assert out[i, :len(x)].tobytes() == x.tobytes()
            continue
        ref, mass = reference(x, orig, new)
        if i >= len(lengths):                                   # an impulse: the coefficients themselves, to one fp32 ulp
            assert (np.abs(got - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
        bound = (plan.T + 2) * 2.0 ** -24 * mass + TINY
        worst = max(worst, float((np.abs(got - ref) / bound).max()) if len(ref) else 0.0)
    print(f"resample {orig} -> {new}: T = {plan.T}, P = {plan.P}, lds = {plan.lds_bytes} B, worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_mixed_batch_gives_the_bits_of_the_single_pair_calls_on_every_run(resamplers):
    g = np.random.default_rng(5)
    spans = [resamplers[new].plan(orig).P * resamplers[new].plan(orig).o for orig, new in PAIRS]
    rows = [g.standard_normal(k + 1).astype(np.float32) for k in spans]
    stride = max(new_length(resamplers, p, len(r)) for r, p in zip(rows, PAIRS)) + 3
    out, nout = launch(resamplers, rows, PAIRS, stride)
    again, _ = launch(resamplers, rows, PAIRS, stride)
    assert out.tobytes() == again.tobytes()
    for i, (r, p) in enumerate(zip(rows, PAIRS)):
        alone, k = launch(resamplers, [r], [p], stride)
        assert k[0] == nout[i] and alone[0].tobytes() == out[i].tobytes()


def test_refusals_return_their_code_and_write_nothing(resamplers):
    from vipant_amd import _ffi
    rs = resamplers[16000]
    classes = (_ffi.ResampleClass * 1)(rs._class(48000))
    wave = torch.zeros(2, 64, device=DEV)
    ns = torch.full((2,), 64, dtype=torch.int64, device=DEV)
    out = torch.full((2, 24), float("nan"), device=DEV)
    nout = torch.full((2,), -77, dtype=torch.int64, device=DEV)
    ok, bad = (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(0, 1)
    args = lambda **kw: [kw.get(k, v) for k, v in dict(wave=wave.data_ptr(), ws=64, ns=ns.data_ptr(), cls=ok, classes=classes, nc=1,
                                                       out=out.data_ptr(), os=24, nout=nout.data_ptr(), b=2, stream=None).items()]
    for why, kw in (("NULL", dict(wave=None)), ("NULL", dict(nout=None)), (r"b = 0", dict(b=0)), ("strides", dict(os=0)),
                    ("overlaps", dict(out=wave.data_ptr() + 64)), ("class 1 outside", dict(cls=bad)), ("classes outside", dict(nc=0))):
        with pytest.raises(_ffi.VipantError, match=f"code -1.*{why}"):
            _ffi.call("vipant_resample", *args(**kw))
    assert bool(torch.isnan(out).all()) and nout.tolist() == [-77, -77] and not bool(wave.any())
    _ffi.call("vipant_resample", *args())
    assert nout.tolist() == [22, 22] and not bool(torch.isnan(out).any())
