"""`vipant_pcm_wave` / `frontend.pcm_wave`: decoded 16-bit interleaved PCM -> the fp32 mono waveform, against the torch CPU expressions
it stands for -- bit for bit: `first` is channel 0 of torchaudio.load(normalize=True), i.e. x[:, 0].float() / 32768, `mean` is
(x.float() / 32768).mean over the channels.  One small ragged batch (b = 6, at most 4 097 frames) covers channels 1, 2, 3, 6, 8,
lengths 0, 1, 63, 64, 65, 4 097 and the planted extremes; the raw ABI calls cover guard rows, strides and pointers that defeat the
16-byte path, tiling, and device values out of range."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHANNELS = [1, 2, 3, 6, 8, 2]
LENGTHS = [4097, 65, 64, 63, 1, 0]


def _clips(seed=5, channels=CHANNELS, lengths=LENGTHS):
    g = np.random.default_rng(seed)
    clips = []
    for ch, n in zip(channels, lengths):
        x = g.integers(-32768, 32768, size=(n, ch), dtype=np.int64).astype(np.int16)
        if n > 4:
            x[0, :], x[1, :], x[2, :], x[3, :] = -32768, 32767, -1, 1
            x[n - 1, 0] = -32768
        clips.append(x)
    return clips


def _pack(clips, stride=None, offset=0):
    """-> (a flat int16 device buffer, the [b, stride] view into it starting `offset` elements in, nframes, channels)."""
    b = len(clips)
    need = max(max((c.size for c in clips), default=1), 1)
    stride = stride if stride is not None else -(-need // 8) * 8
    flat = torch.full((b * stride + offset + 16,), 12345, dtype=torch.int16)
    view = flat[offset:offset + b * stride].view(b, stride)
    view.zero_()
    for i, c in enumerate(clips):
        view[i, :c.size] = torch.from_numpy(c.reshape(-1).copy())
    flat = flat.to(DEV)
    return flat, flat[offset:offset + b * stride].view(b, stride), torch.tensor([c.shape[0] for c in clips]), torch.tensor(
        [c.shape[1] for c in clips], dtype=torch.int32)


def _expect(x, mode):
    """The torch CPU expression for one clip int16 [n, ch] -> fp32 [n]."""
    w = torch.from_numpy(x.T.copy()).float() / 32768           # [ch, n], as torchaudio.load(normalize=True) returns it
    return w[0] if mode == "first" else w.mean(0)


def _tiled(w, tile_len):
    n = w.shape[0]
    if tile_len > 0 and 0 < n < tile_len:
        return torch.tile(w.unsqueeze(0), (1, int(np.ceil(tile_len / n))))[:tile_len][0]      # the reference's slice cuts nothing
    return w


def _raw(pcm, nframes, channels, mode, tile_len, wave_stride, guard=2, wave_offset=0):
    """The ABI call into a NaN-filled buffer with guard rows before and after -> (wave [b, wave_stride], nsamples, the guards)."""
    from vipant_amd import _ffi
    b, stride = pcm.shape
    buf = torch.full(((b + 2 * guard) * wave_stride + wave_offset + 8,), float("nan"), device=DEV)
    lo = guard * wave_stride + wave_offset
    nf = nframes.to(DEV, torch.int64)
    chn = channels.to(DEV, torch.int32)
    nout = torch.full((b + 2,), -7, dtype=torch.int64, device=DEV)
    _ffi.call("vipant_pcm_wave", pcm.data_ptr(), stride, nf.data_ptr(), chn.data_ptr(), {"first": 0, "mean": 1}[mode], tile_len,
              buf.data_ptr() + 4 * lo, wave_stride, nout.data_ptr() + 8, b, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    buf, nout = buf.cpu(), nout.cpu()
    assert nout[0] == -7 and nout[-1] == -7
    outside = torch.cat([buf[:lo], buf[lo + b * wave_stride:]])
    assert bool(torch.isnan(outside).all()), "a guard element was written"
    return buf[lo:lo + b * wave_stride].view(b, wave_stride), nout[1:-1]


def _check(wave, nsamples, want):
    for i, w in enumerate(want):
        n = min(w.shape[0], wave.shape[1])
        assert int(nsamples[i]) == n, (i, int(nsamples[i]), n)
        assert torch.equal(wave[i, :n].view(torch.int32), w[:n].contiguous().view(torch.int32)), i      # the bits, -0.0 included
        assert bool((wave[i, n:].view(torch.int32) == 0).all()), i


@pytest.mark.parametrize("mode", ["first", "mean"])
def test_ragged_batch_bit_for_bit(mode):
    from vipant_amd.frontend import pcm_wave
    clips = _clips()
    _, pcm, nframes, channels = _pack(clips)
    want = [_expect(c, mode) for c in clips]
    wave, nsamples = pcm_wave(pcm, nframes, channels, mode=mode)
    assert wave.dtype == torch.float32 and wave.shape == (6, pcm.shape[1]) and nsamples.dtype == torch.int64
    _check(wave.cpu(), nsamples.cpu(), want)
    again, nagain = pcm_wave(pcm, nframes, channels, mode=mode)
    assert torch.equal(again.view(torch.int32), wave.view(torch.int32)) and torch.equal(nagain, nsamples)      # two runs, the same bits
    if mode == "mean":       # the planted extremes survive the mean: every channel holds them
        for i in (0, 1, 2):
            assert wave[i, :4].tolist() == [-1.0, 32767 / 32768, -1 / 32768, 1 / 32768]


@pytest.mark.parametrize("mode", ["first", "mean"])
@pytest.mark.parametrize("stride_pad,offset,wave_stride,wave_offset", [(0, 0, 4104, 0), (3, 0, 4101, 0), (0, 1, 4104, 1), (5, 3, 4099, 3)])
def test_guards_strides_and_misaligned_pointers(mode, stride_pad, offset, wave_stride, wave_offset):
    clips = _clips(seed=6)
    need = max(c.size for c in clips)
    _, pcm, nframes, channels = _pack(clips, stride=-(-need // 8) * 8 + stride_pad, offset=offset)
    assert pcm.data_ptr() % 16 == (2 * offset) % 16
    wave, nsamples = _raw(pcm, nframes, channels, mode, 0, wave_stride, wave_offset=wave_offset)
    _check(wave, nsamples, [_expect(c, mode) for c in clips])


def test_a_clip_longer_than_the_output_is_cut():
    clips = _clips(seed=7)
    _, pcm, nframes, channels = _pack(clips)
    wave, nsamples = _raw(pcm, nframes, channels, "mean", 0, 61)
    _check(wave, nsamples, [_expect(c, "mean") for c in clips])
    assert nsamples.tolist() == [61, 61, 61, 61, 1, 0]


@pytest.mark.parametrize("mode", ["first", "mean"])
def test_tiling(mode):
    from vipant_amd.frontend import pcm_wave
    clips = _clips(seed=8, channels=[1, 2, 3, 2, 1], lengths=[100, 4096, 4097, 7, 0])
    _, pcm, nframes, channels = _pack(clips)
    want = [_tiled(_expect(c, mode), 4096) for c in clips]
    assert [w.shape[0] for w in want] == [4100, 4096, 4097, 4102, 0]
    wave, nsamples = _raw(pcm, nframes, channels, mode, 4096, 4104)
    _check(wave, nsamples, want)
    assert nsamples.tolist() == [4100, 4096, 4097, 4102, 0]
    assert torch.equal(wave[0, :4100].view(41, 100), wave[0, :100].expand(41, 100))          # periodic
    clamped, nclamped = _raw(pcm, nframes, channels, mode, 4096, 4098)                      # a tiled length above wave_stride
    _check(clamped, nclamped, want)
    assert nclamped.tolist() == [4098, 4096, 4097, 4098, 0]
    auto, nauto = pcm_wave(pcm, nframes, channels, mode=mode, tile_len=4096)                # the default width holds every tiling
    assert auto.shape[1] >= 4102
    _check(auto.cpu(), nauto.cpu(), want)


def test_device_values_out_of_range_are_clamped():
    """nframes -3 and 10^9, channels 0 and 99: nothing outside `pcm` is read (the rows behind the view hold a sentinel that would
    show), and the result is that of the clamped values."""
    g = np.random.default_rng(9)
    stride = 72
    rows = g.integers(-32768, 32768, size=(4, stride), dtype=np.int64).astype(np.int16)
    flat = torch.full((stride * 6,), 12345, dtype=torch.int16)
    flat[stride:5 * stride] = torch.from_numpy(rows.reshape(-1).copy())
    flat = flat.to(DEV)
    pcm = flat[stride:5 * stride].view(4, stride)
    nframes = torch.tensor([-3, 10 ** 9, 10 ** 9, 20])
    channels = torch.tensor([2, 0, 99, 99], dtype=torch.int32)
    for mode in ("first", "mean"):
        wave, nsamples = _raw(pcm, nframes, channels, mode, 0, 80)
        want = [torch.zeros(0), _expect(rows[1].reshape(72, 1), mode), _expect(rows[2].reshape(9, 8), mode),
                _expect(rows[3].reshape(9, 8), mode)]
        _check(wave, nsamples, want)
        assert nsamples.tolist() == [0, 72, 9, 9]


def test_the_wrapper_refuses_what_it_cannot_run():
    from vipant_amd._ffi import VipantError
    from vipant_amd.frontend import pcm_wave
    pcm = torch.zeros(2, 16, dtype=torch.int16, device=DEV)
    n, ch = torch.tensor([4, 4]), torch.tensor([1, 2], dtype=torch.int32)
    with pytest.raises(VipantError, match="int16"):
        pcm_wave(pcm.float(), n, ch)
    with pytest.raises(VipantError, match="no CPU path"):
        pcm_wave(pcm.cpu(), n, ch)
    with pytest.raises(VipantError, match="mode"):
        pcm_wave(pcm, n, ch, mode="left")
    with pytest.raises(VipantError, match="shape"):
        pcm_wave(pcm, n[:1], ch)
