"""Waveform mixup with partner rows OUTSIDE the batch (vipant_fbank_mix_src, KaldiFbank(..., mix=, outputs=)): wave holds nsrc >= b
rows, rows 0 .. b-1 produce the b log-mels, rows b .. nsrc-1 are only read as partners.

Three bit contracts and one tolerance:
  (a) nsrc == b gives vipant_fbank_mix's bits;
  (b) for any partner layout the result is rows 0 .. b-1 of vipant_fbank_mix over all nsrc rows with mix_index -1 for rows >= b,
      bit for bit, and two runs are identical;
  (c) against oracle/fbank_cpu.py on the reference-order mixed waveform the tolerances of tests/test_fbank_mix_gpu.py apply as they
      stand (2e-3 + MIX_MAX, 5e-5 + MIX_MEAN, 5e-4 + MIX_NORM): the clips are that file's four, the partner rows are copies of
      them and the lambdas are the same, so every mixed waveform here is one of that file's (same clip, same partner samples, same
      lambda) and the oracle's own fp32-vs-fp64 distance measured there covers it.

Shapes: test_fbank_mix_gpu.py's three (transform sizes 512 / 2048 / 1024); b = 4, nsrc = 4, 5 and 8."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import fbank_cpu as FB  # noqa: E402
from test_fbank_mix_gpu import LAMBDA, MIX_MAX, MIX_MEAN, MIX_NORM, SHAPES, clips, mixed_wave  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 4
# partner layouts; rows 4 .. 7 are copies of clips 1, 0, 2, 3 (lengths n - 3001, n, n - 17, n).  Every (clip, partner clip, lambda) is
# one of test_fbank_mix_gpu.py's: clip 0 <- clip 1 (shorter), clip 1 <- clip 0 (longer), clip 2 unmixed, clip 3 <- clip 0 (equal length)
COPY_OF = [0, 1, 2, 3, 1, 0, 2, 3]
LAYOUTS = {
    4: [1, 0, -1, 0],            # all partners in the batch: vipant_fbank_mix's own case
    5: [4, 0, -1, 0],            # clip 0 <- outside row 4 (shorter); clips 1 and 3 <- clip 0 in the batch, which is itself mixed
    8: [4, 5, -1, 5],            # all partners outside: shorter, longer, equal length; rows 6 and 7 are pointed at by nobody
}


def sources(sr, n, nsrc):
    w, lens = clips(sr, n, seed=sr)
    rows = COPY_OF[:nsrc]
    return w[rows].contiguous(), lens[rows].contiguous()


_oracle = {}


def oracle(sr, n, T, F, norms=(), masks=None):
    """The CPU filter bank on the reference-order mixed waveform of the four clips; computed once per shape, never changed."""
    key = (sr, n, T, F, norms, None if masks is None else tuple(map(tuple, masks.tolist())))
    if key not in _oracle:
        w, lens = clips(sr, n, seed=sr)
        index, lam = torch.tensor(LAYOUTS[4]), torch.tensor(LAMBDA)
        rows = []
        for i in range(B):
            kw = {}
            if masks is not None:
                f0, f1, t0, t1 = masks[i].tolist()
                kw = dict(freq_mask=(f0, f1), time_mask=(t0, t1))
            rows.append(FB.spectrogram_item(mixed_wave(w, lens, i, index, lam), sr, T, F, norms=norms, zero_mean_wf=False, **kw))
        _oracle[key] = torch.stack(rows)
    return _oracle[key]


def mix_of(nsrc, index=None):
    return torch.tensor(LAYOUTS[nsrc] if index is None else index, dtype=torch.int32), torch.tensor(LAMBDA, dtype=torch.float32)


def concat_mix(nsrc, index):
    """mix arguments of vipant_fbank_mix over all nsrc rows: rows >= b unmixed."""
    full_i = torch.full((nsrc,), -1, dtype=torch.int32)
    full_l = torch.ones((nsrc,), dtype=torch.float32)
    full_i[:B] = index
    full_l[:B] = torch.tensor(LAMBDA)
    return full_i, full_l


@pytest.mark.parametrize("sr,n,T,F", SHAPES)
def test_nsrc_equal_b_is_fbank_mix_bit_for_bit(sr, n, T, F):
    """(a): the entry point itself at nsrc == b (the frontend keeps calling vipant_fbank_mix there), and the keyword with nsrc == b."""
    from vipant_amd import _ffi, ops
    from vipant_amd.frontend import KaldiFbank
    w, lens = sources(sr, n, 4)
    w, lens = w.to(DEV), lens.to(DEV)
    index, lam = mix_of(4)
    fb = KaldiFbank(sr, F, T, norms=(), device=DEV)
    want = fb(w, lens, mix=(index, lam))
    assert torch.equal(fb(w, lens, mix=(index, lam), outputs=4), want)
    out = torch.full((B, 1, T, F), float("nan"), device=DEV)
    ws = ops.scratch("fbank", _ffi.query("vipant_fbank_mix_src_workspace_bytes", 4, 4), torch.device(DEV))
    assert _raw(fb, w, lens, out.data_ptr(), index.to(DEV), lam.to(DEV), 4, B, T, ws) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)


@pytest.mark.parametrize("nsrc", [5, 8])
@pytest.mark.parametrize("sr,n,T,F", SHAPES)
def test_outside_partners_equal_the_concatenated_batch_and_the_oracle(sr, n, T, F, nsrc):
    """(b) and (c)."""
    from vipant_amd.frontend import KaldiFbank
    w, lens = sources(sr, n, nsrc)
    w, lens = w.to(DEV), lens.to(DEV)
    index, lam = mix_of(nsrc)
    fb = KaldiFbank(sr, F, T, norms=(), device=DEV)
    got = fb(w, lens, mix=(index, lam), outputs=B)
    again = fb(w, lens, mix=(index, lam), outputs=B)
    assert got.shape == (B, 1, T, F)
    assert torch.equal(got, again)
    whole = fb(w, lens, mix=concat_mix(nsrc, index))
    assert whole.shape == (nsrc, 1, T, F)
    assert torch.equal(got, whole[:B])
    assert not torch.equal(got[0], fb(w[:B], lens[:B])[0])              # clip 0 really is mixed
    ref = oracle(sr, n, T, F)
    got = got.cpu()
    for i in range(B):
        err = (got[i, 0] - ref[i]).abs()
        print(f"sr {sr} nsrc {nsrc} clip {i}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
        assert err.max() < 2e-3 + MIX_MAX, (i, float(err.max()))
        assert err.mean() < 5e-5 + MIX_MEAN, (i, float(err.mean()))


def test_outside_partners_with_norms_and_masks():
    from vipant_amd.frontend import KaldiFbank
    sr, n, T, F = SHAPES[0]
    w, lens = sources(sr, n, 8)
    w, lens = w.to(DEV), lens.to(DEV)
    index, lam = mix_of(8)
    fb = KaldiFbank(sr, F, T, norms=(-4.94, 5.76), freq_mask_param=16, time_mask_param=40, device=DEV)
    masks = fb.draw_masks(B, generator=torch.Generator().manual_seed(11))
    got = fb(w, lens, masks, mix=(index, lam), outputs=B)
    full_masks = torch.zeros((8, 4), dtype=masks.dtype)
    full_masks[:B] = masks
    whole = fb(w, lens, full_masks, mix=concat_mix(8, index))
    assert torch.equal(got, whole[:B])
    ref = oracle(sr, n, T, F, norms=(-4.94, 5.76), masks=masks)
    err = (got.cpu()[:, 0] - ref).abs().amax(dim=(1, 2))
    print("norms+masks, outside partners: max per clip", [f"{float(e):.3e}" for e in err])
    assert bool((err < 5e-4 + MIX_NORM).all()), err.tolist()


def _raw(fb, t_wave, t_lens, out_ptr, t_index, t_lam, nsrc, b, T, t_ws, **over):
    """vipant_fbank_mix_src itself, with the pointers and sizes the caller chooses (`over` replaces an argument) -> status code."""
    from vipant_amd import _ffi, ops
    a = dict(wave=t_wave.data_ptr(), stride=t_wave.shape[1], lens=t_lens.data_ptr(), out=out_ptr, window=fb.window.data_ptr(),
             banks=fb.banks.data_ptr(), bank_start=fb.bank_start.data_ptr(), bank_len=fb.bank_len.data_ptr(), index=t_index.data_ptr(),
             lam=t_lam.data_ptr(), F=fb.num_mel_bins, nfft=fb.padded, ws=t_ws.data_ptr(), ws_bytes=t_ws.numel())
    a.update(over)
    return _ffi.lib().vipant_fbank_mix_src(a["wave"], a["stride"], a["lens"], a["out"], a["window"], a["banks"], a["bank_start"],
                                           a["bank_len"], None, a["index"], a["lam"], nsrc, b, T, a["F"], fb.size, fb.shift, a["nfft"],
                                           fb.preemphasis, 0.0, 0.0, a["ws"], a["ws_bytes"], ops._stream())


@pytest.mark.parametrize("nsrc", [4, 5, 8])
def test_out_of_range_partner_is_clamped(nsrc):
    """(d): nsrc and 10^6 become row nsrc - 1; -5 and INT_MIN become "not mixed"."""
    from vipant_amd.frontend import KaldiFbank
    sr, n, T, F = SHAPES[0]
    w, lens = sources(sr, n, nsrc)
    w, lens = w.to(DEV), lens.to(DEV)
    fb = KaldiFbank(sr, F, T, norms=(), device=DEV)
    lam = torch.tensor(LAMBDA)
    wild = torch.tensor([nsrc, 1000000, -5, -2147483648], dtype=torch.int32)
    want = torch.tensor([nsrc - 1, nsrc - 1, -1, -1], dtype=torch.int32)
    if nsrc == B:                                                       # the frontend goes to vipant_fbank_mix here: call the entry itself
        from vipant_amd import _ffi, ops
        ws = ops.scratch("fbank", _ffi.query("vipant_fbank_mix_src_workspace_bytes", nsrc, B), torch.device(DEV))
        got = torch.full((B, 1, T, F), float("nan"), device=DEV)
        assert _raw(fb, w, lens, got.data_ptr(), wild.to(DEV), lam.to(DEV), nsrc, B, T, ws) == 0
        torch.cuda.synchronize()
    else:
        got = fb(w, lens, mix=(wild, lam), outputs=B)
    assert torch.equal(got, fb(w, lens, mix=(want, lam), outputs=B))
    assert torch.equal(got[2], fb(w[:B], lens[:B])[2]) and torch.equal(got[3], fb(w[:B], lens[:B])[3])


def test_refusals_write_nothing_and_a_good_call_stays_inside_out():
    """(e)"""
    from vipant_amd import _ffi, ops
    from vipant_amd.frontend import KaldiFbank
    sr, n, T, F = SHAPES[0]
    nsrc = 8
    w, lens = sources(sr, n, nsrc)
    w, lens = w.to(DEV), lens.to(DEV)
    fb = KaldiFbank(sr, F, T, norms=(), device=DEV)
    need = _ffi.query("vipant_fbank_mix_src_workspace_bytes", nsrc, B)
    assert need >= (nsrc + B) * 4 and _ffi.query("vipant_fbank_mix_src_workspace_bytes", B, B) == _ffi.query("vipant_fbank_mix_workspace_bytes", B)
    ws = ops.scratch("fbank", need, torch.device(DEV))
    guard = 2 * T * F
    buf = torch.full((guard + B * T * F + guard,), -777.0, device=DEV)
    out_ptr = buf.data_ptr() + 4 * guard
    index, lam = mix_of(nsrc)
    index, lam = index.to(DEV), lam.to(DEV)

    def raw(nsrc=nsrc, b=B, T=T, **over):
        return _raw(fb, w, lens, out_ptr, index, lam, nsrc, b, T, ws, **over)

    for name in ("wave", "lens", "out", "window", "banks", "bank_start", "bank_len", "index", "lam", "ws"):
        assert raw(**{name: None}) != 0, name                           # a NULL argument
    assert raw(b=0) != 0 and raw(b=-1) != 0                             # b < 1
    assert raw(nsrc=3) != 0 and raw(nsrc=0) != 0                        # nsrc < b
    assert raw(stride=0) != 0 and raw(stride=-16000) != 0               # stride < 1
    assert raw(T=0) != 0 and raw(F=0) != 0 and raw(F=257) != 0          # bad T / F
    assert raw(nfft=500) != 0 and raw(nfft=4096) != 0 and raw(nfft=256) != 0
    assert raw(ws_bytes=need - 256) != 0                                # workspace too small
    torch.cuda.synchronize()
    assert bool((buf == -777.0).all())
    assert raw() == 0
    torch.cuda.synchronize()
    body = buf[guard:guard + B * T * F].view(B, 1, T, F)
    assert bool(torch.isfinite(body).all()) and bool((body != -777.0).all())
    assert bool((buf[:guard] == -777.0).all()) and bool((buf[guard + B * T * F:] == -777.0).all())
    assert torch.equal(body, fb(w, lens, mix=(index, lam), outputs=B))
    with pytest.raises(_ffi.VipantError):
        fb(w, lens, mix=(index, lam), outputs=9)                        # more outputs than rows
    with pytest.raises(_ffi.VipantError):
        fb(w, lens, mix=(index, lam), outputs=0)
    with pytest.raises(_ffi.VipantError):
        fb(w, lens, outputs=B)                                          # outputs without mix
    with pytest.raises(_ffi.VipantError):
        fb(w, lens, mix=(torch.full((8,), -1, dtype=torch.int32), torch.ones(8)), outputs=B)      # draws not [outputs]


def test_unreferenced_partner_rows_do_not_reach_out():
    """(f): rows >= b full of NaN, none of them pointed at."""
    from vipant_amd.frontend import KaldiFbank
    sr, n, T, F = SHAPES[0]
    w, lens = sources(sr, n, 8)
    index, lam = mix_of(8)                                              # points at rows 4 and 5 only
    fb = KaldiFbank(sr, F, T, norms=(), device=DEV)
    want = fb(w.to(DEV), lens.to(DEV), mix=(index, lam), outputs=B)
    w[6:] = float("nan")
    got = fb(w.to(DEV), lens.to(DEV), mix=(index, lam), outputs=B)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    w[4:] = float("nan")
    inside = torch.tensor([1, 0, -1, 0], dtype=torch.int32)             # partners in the batch: no outside row is pointed at
    got = fb(w.to(DEV), lens.to(DEV), mix=(inside, lam), outputs=B)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, fb(w[:B].to(DEV), lens[:B].to(DEV), mix=(inside, lam)))
