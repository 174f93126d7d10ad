"""Waveform mixup inside the log-mel launch (vipant_fbank_mix, KaldiFbank(..., mix=)) against the CPU filter bank of
oracle/fbank_cpu.py fed with the waveform the reference forms (cvap/data/audioset_cls.py:374-398) in torch fp32.

Tolerance: tests/test_frontend_gpu.py's (max 2e-3, mean 5e-5 without norms; 5e-4 with norms and masks) plus what the mixing
arithmetic itself contributes, measured on the CPU as oracle(fp32 mix) against oracle(fp64 mix) on these very clips: over the
three shapes and twelve clips below the largest figures are max 2.08e-4 and mean 9.1e-7 without norms (MIX_MAX, MIX_MEAN) and
2.08e-4 / 5.76 = 3.6e-5 after the (x + 4.94) / 5.76 normalisation (MIX_NORM).  The large single entries are nearly empty filters
near the log floor.

The issue's two shapes both have an odd log2 transform size (512, 2048); (32000, 32000, 128, 80) adds the even one (1024)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import fbank_cpu as FB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIX_MAX, MIX_MEAN, MIX_NORM = 2.1e-4, 9.1e-7, 3.7e-5
SHAPES = [(16000, 16000, 128, 64), (44100, 57330, 128, 128), (32000, 32000, 128, 80)]
INDEX = [1, 0, -1, 0]            # clip 0 <- shorter partner, 1 <- longer partner (itself mixed), 2 unmixed, 3 <- equal length (itself mixed)
LAMBDA = [0.43, 0.61, 1.0, 0.5]


def clips(sr, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / float(sr)
    w = 0.05 * torch.randn(4, n, generator=g)
    for i in range(4):
        f0 = 200.0 + 700.0 * i
        w[i] += 0.3 * torch.sin(2 * torch.pi * f0 * t) + 0.1 * torch.sin(2 * torch.pi * 3.1 * f0 * t) + 0.02 * (i - 1)
    return w, torch.tensor([n, n - 3001, n - 17, n])


def mixed_wave(w, lens, i, index, lam, dtype=torch.float32):
    """audioset_cls.py:374-398 for clip i: zero-mean clip, zero-mean ORIGINAL partner cut / zero-padded to the clip, mixed, zero-mean."""
    wf = w[i, :int(lens[i])].to(dtype)
    wf = wf - wf.mean()
    p = int(index[i])
    if p < 0:
        return wf
    wf_mix = w[p, :int(lens[p])].to(dtype)
    wf_mix = wf_mix - wf_mix.mean()
    wf_mix = wf_mix[:wf.shape[0]]
    npad = wf.shape[0] - wf_mix.shape[0]
    if npad > 0:
        wf_mix = torch.nn.functional.pad(wf_mix, (0, npad), mode="constant", value=0.)
    lambd = float(lam[i])
    wf_mixed = lambd * wf + (1 - lambd) * wf_mix
    return wf_mixed - wf_mixed.mean()


def mix_args():
    return torch.tensor(INDEX, dtype=torch.int32), torch.tensor(LAMBDA, dtype=torch.float32)


@pytest.mark.parametrize("sr,n,T,F", SHAPES)
def test_mix_matches_oracle_and_unmixed_clips_keep_their_bits(sr, n, T, F):
    from vipant_amd.frontend import KaldiFbank
    w, lens = clips(sr, n, seed=sr)
    index, lam = mix_args()
    fb = KaldiFbank(sr, F, T, norms=(), device=DEV)
    got = fb(w.to(DEV), lens.to(DEV), mix=(index, lam))
    again = fb(w.to(DEV), lens.to(DEV), mix=(index, lam))
    plain = fb(w.to(DEV), lens.to(DEV))
    assert got.shape == (4, 1, T, F)
    assert torch.equal(got, again)                                     # fixed-order reductions: two runs, same bits
    assert torch.equal(got[2], plain[2])                               # mix_index -1: vipant_fbank(zero_mean=1)'s bits
    assert not torch.equal(got[0], plain[0])
    got = got.cpu()
    for i in range(4):
        ref = FB.spectrogram_item(mixed_wave(w, lens, i, index, lam), sr, T, F, norms=(), zero_mean_wf=False)
        err = (got[i, 0] - ref).abs()
        print(f"sr {sr} clip {i}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}")
        assert err.max() < 2e-3 + MIX_MAX, (i, float(err.max()))
        assert err.mean() < 5e-5 + MIX_MEAN, (i, float(err.mean()))


def test_mix_with_norms_and_masks():
    from vipant_amd.frontend import KaldiFbank
    sr, n, T, F = SHAPES[0]
    w, lens = clips(sr, n, seed=sr)
    index, lam = mix_args()
    fb = KaldiFbank(sr, F, T, norms=(-4.94, 5.76), freq_mask_param=16, time_mask_param=40, device=DEV)
    masks = fb.draw_masks(4, generator=torch.Generator().manual_seed(11))
    got = fb(w.to(DEV), lens.to(DEV), masks, mix=(index, lam)).cpu()
    for i in range(4):
        f0, f1, t0, t1 = masks[i].tolist()
        ref = FB.spectrogram_item(mixed_wave(w, lens, i, index, lam), sr, T, F, norms=(-4.94, 5.76), zero_mean_wf=False,
                                  freq_mask=(f0, f1), time_mask=(t0, t1))
        err = (got[i, 0] - ref).abs().max()
        print(f"norms+masks clip {i}: max {float(err):.3e}")
        assert err < 5e-4 + MIX_NORM, (i, float(err))
    nfr = fb.num_frames(int(lens[0]))
    assert nfr == 98
    pad_val = (0.0 - (-4.94)) / 5.76
    keep = torch.ones(T, F, dtype=torch.bool)
    keep[:, masks[0, 0]:masks[0, 1]] = False
    keep[masks[0, 2]:masks[0, 3], :] = False
    assert torch.allclose(got[0, 0][nfr:][keep[nfr:]], torch.tensor(pad_val), atol=1e-6)


def _raw(fb, wave, lens, out_ptr, index_ptr, lam_ptr, b, T, ws):
    """vipant_fbank_mix itself, with the pointers the caller chooses -> status code."""
    from vipant_amd import _ffi, ops
    return _ffi.lib().vipant_fbank_mix(wave.data_ptr(), wave.shape[1], lens.data_ptr(), out_ptr, fb.window.data_ptr(), fb.banks.data_ptr(),
                                       fb.bank_start.data_ptr(), fb.bank_len.data_ptr(), None, index_ptr, lam_ptr, b, T, fb.num_mel_bins,
                                       fb.size, fb.shift, fb.padded, fb.preemphasis, 0.0, 0.0, ws.data_ptr(), ws.numel(), ops._stream())


def test_out_of_range_partner_is_clamped_and_refusals_write_nothing():
    from vipant_amd import _ffi, ops
    from vipant_amd.frontend import KaldiFbank
    sr, n, T, F = SHAPES[0]
    w, lens = clips(sr, n, seed=sr)
    w, lens = w.to(DEV), lens.to(DEV)
    fb = KaldiFbank(sr, F, T, norms=(), device=DEV)
    ws = ops.scratch("fbank", _ffi.query("vipant_fbank_mix_workspace_bytes", 4), torch.device(DEV))
    guard = 2 * T * F
    buf = torch.full((guard + 4 * T * F + guard,), -777.0, device=DEV)
    out_ptr = buf.data_ptr() + 4 * guard
    index = torch.tensor([4, 1000000, -5, -2147483648], dtype=torch.int32, device=DEV)       # host cannot see these: the kernel clamps
    lam = torch.tensor(LAMBDA, device=DEV)
    # refusals first: the buffer must still be all sentinel afterwards
    assert _raw(fb, w, lens, out_ptr, index.data_ptr(), None, 4, T, ws) != 0                  # null mix_lambda
    assert _raw(fb, w, lens, out_ptr, None, lam.data_ptr(), 4, T, ws) != 0                    # null mix_index
    assert _raw(fb, w, lens, out_ptr, index.data_ptr(), lam.data_ptr(), 0, T, ws) != 0        # b = 0
    assert _raw(fb, w, lens, out_ptr, index.data_ptr(), lam.data_ptr(), 4, 0, ws) != 0        # T = 0
    torch.cuda.synchronize()
    assert bool((buf == -777.0).all())
    assert _raw(fb, w, lens, out_ptr, index.data_ptr(), lam.data_ptr(), 4, T, ws) == 0
    torch.cuda.synchronize()
    body = buf[guard:guard + 4 * T * F].view(4, T, F)
    assert bool(torch.isfinite(body).all()) and bool((body != -777.0).all())
    assert bool((buf[:guard] == -777.0).all()) and bool((buf[guard + 4 * T * F:] == -777.0).all())
    # above the range clamps to the last clip, below -1 to "not mixed"
    want = fb(w, lens, mix=(torch.tensor([3, 3, -1, -1], dtype=torch.int32), lam))
    assert torch.equal(body, want[:, 0])
    with pytest.raises(_ffi.VipantError):
        fb(w, lens, mix=(torch.tensor([0, 1], dtype=torch.int32), lam))                      # shape of the draws != [b]


def test_draw_mixup():
    from vipant_amd.frontend import KaldiFbank
    a = KaldiFbank.draw_mixup(64, 0.5, torch.Generator().manual_seed(3))
    b = KaldiFbank.draw_mixup(64, 0.5, torch.Generator().manual_seed(3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    index, lam = a
    assert index.dtype == torch.int32 and lam.dtype == torch.float32
    mixed = index >= 0
    assert 10 < int(mixed.sum()) < 54 and bool((index < 64).all()) and bool((index[mixed] != torch.arange(64)[mixed]).all())
    assert bool((lam[~mixed] == 1).all()) and bool(((lam[mixed] > 0.1) & (lam[mixed] < 0.9)).all())
    assert bool((KaldiFbank.draw_mixup(16, 0.0, torch.Generator().manual_seed(1))[0] == -1).all())
    assert KaldiFbank.draw_mixup(1, 1.0, torch.Generator().manual_seed(1))[0].tolist() == [-1]
