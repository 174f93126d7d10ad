"""Two masked views from one filter-bank evaluation (vipant_fbank_view_pair; KaldiFbank(..., view=, masks=, masks2=, pair=True)).

The contract is equality: `out` has the bits of vipant_fbank_view under `masks`, `out2` those of vipant_fbank_view under `masks2`, for
the same draws -- the arithmetic of a stored value and its order are those of the single launch, so no tolerance is needed.

Shapes: 16 kHz, b = 5, T = 71 (odd: the last frame pair has no second frame; no multiple of the 32 frames of a workgroup, three
workgroups per clip), F in {40, 64, 128} (below one wave of lanes, exactly one, two strides).  crop_len = 12160 samples.  Clips: 300
samples (shorter than a window: no live frame), 6000 (36 live frames, then padding rows), 12160 (exactly crop_len), 20000 and 17000
(the crop rule; drawn with train = 1, centred with train = 0: both are run).  Mask sets: time masks that start on odd frames and so
split a frame pair, the two views' time masks disjoint, overlapping and nested, one view's time mask over every row, different
frequency masks, masks that reach past T and F, and one view or both without masks.

One case goes against oracle/fbank_cpu.py on the cropped waveform `view_wave` returns, masks applied in numpy, within the project's
bound for that comparison (tests/test_src_trainer_gpu.py, tests/test_wave_view_gpu.py): max 2e-3 and mean 5e-5 plus the oracle's own
distance from a float64 restatement of itself, computed here."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import fbank_cpu as FB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SR, B, T = 16000, 5, 71
CROP_LEN = int((T / 100 + 0.05) * SR)
LENS = [300, 6000, CROP_LEN, 20000, 17000]
STRIDE = 20000
NORMS = (-4.93839311, 5.75751113)
COVER = (0, 0, 0, T)                     # no frequency mask, every row time-masked

# (f0, f1, t0, t1) of view 1 and of view 2 for clip 0; clip i adds i to the time mask's start and end (so that both parities of an
# edge occur in every set) and 2 i to the frequency mask's.  None: the view has no masks.
MASK_SETS = {
    "disjoint": ((3, 10, 5, 13), (20, 33, 21, 30)),
    "overlapping": ((0, 7, 7, 26), (30, 40, 15, 42)),
    "nested": ((5, 6, 3, 50), (8, 30, 11, 20)),
    "nested_the_other_way": ((8, 30, 11, 20), (5, 6, 3, 50)),
    "same_time_mask": ((3, 10, 9, 24), (20, 33, 9, 24)),
    "view1_covers_every_row": (COVER, (2, 9, 9, 12)),
    "view2_covers_every_row": ((2, 9, 9, 12), COVER),
    "past_the_edges": ((30, 400, 65, 71), (0, 1, 66, 90)),
    "view1_none": (None, (20, 33, 21, 30)),
    "view2_none": ((3, 10, 5, 13), None),
    "both_none": (None, None),
}


def masks_of(row):
    if row is None:
        return None
    if row is COVER:
        return torch.tensor([list(COVER)] * B, dtype=torch.int32)
    f0, f1, t0, t1 = row
    return torch.tensor([[f0 + 2 * i, f1 + 2 * i, t0 + i, t1 + i] for i in range(B)], dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def clips():
    """wave [B, STRIDE] on the device, NaN beyond each clip's length; lengths."""
    g = torch.Generator().manual_seed(11)
    t = torch.arange(STRIDE) / SR
    wave = 0.2 * torch.randn(B, STRIDE, generator=g) + 0.1 * torch.sin(2 * np.pi * 440.0 * t)
    wave[4, :6000] *= 0.01                        # a quiet head: the drawn window and the whole clip differ in their deviation
    for i, n in enumerate(LENS):
        wave[i, n:] = float("nan")
    return wave.to(DEV), torch.tensor(LENS).to(DEV)


def frontend(F, train, norms=NORMS, frame_length=25.0):
    from vipant_amd.frontend import KaldiFbank
    return KaldiFbank(SR, F, T, norms=norms, zero_mean_wf=True, frame_length=frame_length, train=train, device=DEV)


def views(fb):
    return fb.draw_views(B, torch.Generator().manual_seed(5))


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("F,norms", [(40, NORMS), (64, ()), (128, NORMS)])
def test_both_views_have_the_bits_of_the_single_launch(F, norms, train):
    fb = frontend(F, train, norms)
    assert fb.crop_len == CROP_LEN and fb.padded == 512
    wave, lens = clips()
    view = views(fb)
    singles = {}

    def single(row):
        if row not in singles:
            singles[row] = fb(wave, lens, masks=masks_of(row), view=view)
            assert bool(torch.isfinite(singles[row]).all())
        return singles[row]

    for name, (r1, r2) in MASK_SETS.items():
        out, out2 = fb(wave, lens, masks=masks_of(r1), view=view, masks2=masks_of(r2), pair=True)
        assert out.shape == out2.shape == (B, 1, T, F) and out.data_ptr() != out2.data_ptr()
        assert torch.equal(out, single(r1)), (name, "view 1")
        assert torch.equal(out2, single(r2)), (name, "view 2")
        if r1 is None and r2 is None:
            assert torch.equal(out, out2)
    # the cases are what they claim to be: clip 0 has no live frame, clip 1 has padding rows, the others none; a covered view is zero
    plain = single(None)[:, 0]
    padv = (0.0 - norms[0]) / norms[1] if norms else 0.0
    assert bool((plain[0] == np.float32(padv)).all()) and bool((plain[1, 36:] == np.float32(padv)).all())
    assert not bool((plain[1, 35] == np.float32(padv)).any()) and not bool((plain[2:, T - 1] == np.float32(padv)).any())
    assert not bool(single(COVER).any())


@pytest.mark.parametrize("frame_length,size", [(50.0, 1024), (100.0, 2048)])
def test_the_longer_transforms(frame_length, size):
    fb = frontend(64, True, frame_length=frame_length)
    assert fb.padded == size
    wave, lens = clips()
    view = views(fb)
    for name in ("overlapping", "nested", "view1_none"):
        r1, r2 = MASK_SETS[name]
        out, out2 = fb(wave, lens, masks=masks_of(r1), view=view, masks2=masks_of(r2), pair=True)
        assert torch.equal(out, fb(wave, lens, masks=masks_of(r1), view=view)), name
        assert torch.equal(out2, fb(wave, lens, masks=masks_of(r2), view=view)), name


def test_view_true_and_the_front_end_refusals():
    from vipant_amd._ffi import VipantError
    fb = frontend(64, False)
    wave, lens = clips()
    m1, m2 = masks_of(MASK_SETS["disjoint"][0]), masks_of(MASK_SETS["disjoint"][1])
    out, out2 = fb(wave, lens, masks=m1, view=True, masks2=m2, pair=True)
    assert torch.equal(out, fb(wave, lens, masks=m1, view=True)) and torch.equal(out2, fb(wave, lens, masks=m2, view=True))
    with pytest.raises(VipantError, match="exclude each other"):
        fb(wave, lens, mix=(torch.tensor([1, 0, -1, -1, -1], dtype=torch.int32), torch.ones(B)), pair=True, view=True)
    with pytest.raises(VipantError, match="needs a view"):
        fb(wave, lens, masks=m1, masks2=m2, pair=True)
    with pytest.raises(VipantError, match="masks2"):
        fb(wave, lens, masks=m1, masks2=m2, view=True)


@pytest.mark.parametrize("F", [40, 128])
def test_every_element_is_written_and_nothing_else(F):
    """Both outputs inside sentinel-filled buffers, the workspace exactly as large as asked, the waveform inside NaN padding."""
    from vipant_amd import _ffi, ops
    fb = frontend(F, True)
    wave, lens = clips()
    view = views(fb)
    r1, r2 = MASK_SETS["overlapping"]
    m1, m2 = masks_of(r1).to(DEV), masks_of(r2).to(DEV)
    want, want2 = fb(wave, lens, masks=m1, view=view), fb(wave, lens, masks=m2, view=view)
    params, draws = fb._view_args(view, B, STRIDE, torch.device(DEV))
    nbytes = _ffi.query("vipant_fbank_view_workspace_bytes", B)
    arena = torch.full((256 + nbytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    ws_ptr = arena.data_ptr() + 256
    n, guard = B * T * F, 2 * T * F
    buf = torch.full((guard + n + guard + n + guard,), -777.0, device=DEV)
    p1, p2 = buf.data_ptr() + 4 * guard, buf.data_ptr() + 4 * (2 * guard + n)
    lib = _ffi.lib()

    def pair(out=p1, out2=p2, wsb=nbytes, k1=m1.data_ptr(), k2=m2.data_ptr()):
        return lib.vipant_fbank_view_pair(wave.data_ptr(), STRIDE, lens.data_ptr(), out, out2, fb.window.data_ptr(), fb.banks.data_ptr(),
                                          fb.bank_start.data_ptr(), fb.bank_len.data_ptr(), k1, k2, B, T, F, fb.size, fb.shift, fb.padded,
                                          fb.preemphasis, NORMS[0], NORMS[1], params, draws.data_ptr(), ws_ptr, wsb, ops._stream())

    # refusals first: both buffers and the workspace must still be all sentinel afterwards
    assert pair(out2=None) != 0
    assert "second output" in lib.vipant_last_error().decode()
    assert pair(out2=p1) != 0 and pair(out2=p1 + 4 * (n - 1)) != 0 and pair(out=p2, out2=p2 - 4 * (n - 1)) != 0
    assert "overlap" in lib.vipant_last_error().decode()
    assert pair(wsb=nbytes - 1) != 0
    assert "workspace" in lib.vipant_last_error().decode()
    assert pair(out=None) != 0
    torch.cuda.synchronize()
    assert bool((buf == -777.0).all()) and bool((arena == 0xA5).all())
    assert pair() == 0
    torch.cuda.synchronize()
    body, body2 = buf[guard:guard + n].view(B, T, F), buf[2 * guard + n:2 * guard + 2 * n].view(B, T, F)
    assert bool(torch.isfinite(body).all()) and bool(torch.isfinite(body2).all())
    assert not bool((body == -777.0).any()) and not bool((body2 == -777.0).any())
    assert torch.equal(body, want[:, 0]) and torch.equal(body2, want2[:, 0])
    for lo, hi in ((0, guard), (guard + n, 2 * guard + n), (2 * guard + 2 * n, 3 * guard + 2 * n)):
        assert bool((buf[lo:hi] == -777.0).all()), (lo, hi)
    assert bool((arena[:256] == 0xA5).all()) and bool((arena[256 + nbytes:] == 0xA5).all())
    # adjacent outputs do not overlap
    buf.fill_(-777.0)
    assert pair(out=p1, out2=p1 + 4 * n) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[guard:guard + n].view(B, T, F), want[:, 0]) and torch.equal(buf[guard + n:guard + 2 * n].view(B, T, F), want2[:, 0])
    assert bool((buf[:guard] == -777.0).all()) and bool((buf[guard + 2 * n:] == -777.0).all())


def _spectrogram64(w, F):
    """oracle.fbank_cpu.spectrogram_item (no norms, zero-mean waveform) restated in float64."""
    w = w.double()
    w = w - w.mean()
    shift, size, padded = FB.window_properties(SR)
    m = FB.num_frames(w.shape[0], size, shift)
    frames = w.as_strided((m, size), (shift, 1)).clone()
    frames = frames - frames.mean(dim=1, keepdim=True)
    prev = torch.cat([frames[:, :1], frames[:, :-1]], dim=1)
    frames = frames - 0.97 * prev
    frames = frames * torch.hann_window(size, periodic=False, dtype=torch.float64).unsqueeze(0)
    frames = torch.nn.functional.pad(frames, (0, padded - size))
    power = torch.fft.rfft(frames, dim=1).abs().pow(2.0)
    mel = power @ FB.mel_banks(F, padded, SR).double().t()
    x = torch.max(mel, torch.tensor(FB.EPS, dtype=torch.float64)).log()[:T]
    return torch.nn.functional.pad(x, (0, 0, 0, T - x.shape[0]))


def test_pair_against_the_cpu_oracle():
    F = 64
    fb = frontend(F, True, norms=())
    wave, lens = clips()
    view = views(fb)
    r1, r2 = MASK_SETS["overlapping"]
    m1, m2 = masks_of(r1), masks_of(r2)
    out, out2 = fb(wave, lens, masks=m1, view=view, masks2=m2, pair=True)
    cropped, nout = fb.view_wave(wave, lens, view)
    cropped, nout = cropped.cpu(), nout.tolist()
    assert nout == [300, 6000, CROP_LEN, CROP_LEN, CROP_LEN]
    for i in range(1, B):
        w = cropped[i, :nout[i]]
        ref = FB.spectrogram_item(w, SR, T, F, norms=(), zero_mean_wf=True)
        own = (ref - _spectrogram64(w, F).float()).abs()
        for got, m, which in ((out, m1, 1), (out2, m2, 2)):
            want = ref.numpy().copy()
            f0, f1, t0, t1 = m[i].tolist()
            want[:, f0:f1] = 0.0
            want[t0:t1, :] = 0.0
            err = np.abs(got[i, 0].cpu().numpy() - want)
            print(f"clip {i} view {which}: max {err.max():.3e} mean {err.mean():.3e}; oracle's own distance max {float(own.max()):.3e} "
                  f"mean {float(own.mean()):.3e}")
            assert err.max() < 2e-3 + float(own.max()), (i, which, float(err.max()))
            assert err.mean() < 5e-5 + float(own.mean()), (i, which, float(err.mean()))
