"""The host side of `running.audio.resample_to`, without a device: the new lengths in exact integers, the class plans of the tested
pairs inside a workgroup's LDS, the refusal of a pair whose table cannot fit, the default of the key, and `AudioBatches` with the key
off (a stub device, as tests/test_audio_batch_cpu.py has it)."""
import math

import pytest
import torch

import test_audio_batch_cpu as AB
from test_audio_batch_cpu import ingests  # noqa: F401  (the fixture: `pcm_wave` / `pcm_ingest` on the host)
from vipant_amd import frontend
from vipant_amd.errors import VipantError

RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)
SEVEN = ((16000, 16000), (48000, 16000), (8000, 16000), (44100, 16000), (11025, 16000), (192000, 16000), (16000, 44100))
TAPS = {(44100, 16000): 34, (11025, 16000): 13, (48000, 16000): 37, (192000, 16000): 145, (8000, 16000): 13}


@pytest.mark.parametrize("orig,new", SEVEN + ((192000, 11025), (11025, 192000)))
def test_lengths_are_exact_integers(orig, new):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    rs = frontend.Resample(new, device="cpu")
    lens = [0, 1, o - 1, o, o + 1, 2 ** 31 // n - 1, 2 ** 31 // n, 2 ** 31 // n + 1, 2 ** 53 // n + 1, 2 ** 40 - 1]
    assert rs.lengths(torch.tensor(lens), orig).tolist() == [-(-n * k // o) for k in lens]
    assert rs.lengths(lens[:2], [orig, new]).tolist() == [0, 1]            # one rate per row; a row at the target keeps its length


@pytest.mark.parametrize("new", RATES)
def test_every_usual_pair_has_a_plan_inside_the_lds_budget(new):
    rs = frontend.Resample(new, device="cpu")
    for orig in RATES:
        c, g = rs.plan(orig), math.gcd(orig, new)
        if orig == new:
            assert (c.T, c.o, c.n) == (0, 1, 1)
            continue
        assert (c.o, c.n) == (orig // g, new // g) and c.T == TAPS.get((orig, new), c.T) and 1 <= c.P and c.P * c.n <= max(4096, 4 * c.n)
        assert c.kmin >= 0 and c.T <= c.kspan <= c.o + c.T + 1
        words = -(-(c.T + 1) * c.n // 4) * 4 + -(-((c.P - 1) * c.o + c.kspan + 3) // 4) * 4
        assert c.lds_bytes == 4 * words <= 160 * 1024


def test_a_pair_with_thousands_of_phases_is_refused_before_any_device_call():
    rs = frontend.Resample(16000, device="cpu")
    with pytest.raises(VipantError, match=r"44101 -> 16000 Hz needs \d+ bytes of LDS"):
        rs.plan(44101)
    with pytest.raises(VipantError, match="44101 -> 16000"):
        rs.lengths([10], 44101)
    with pytest.raises(VipantError, match="phases"):
        frontend.Resample(192000, device="cpu").plan(191999)


@pytest.mark.parametrize("off", [{}, {"resample_to": 0}])
def test_the_key_is_off_by_default_and_then_the_front_ends_are_those_of_before(ingests, off):
    from vipant_amd.config import compose
    assert compose(["+running/audio=default"]).running.audio.resample_to == 0
    for kind, rate in (("pcm", 16000), ("raw", None)):
        ab = AB.Batches((), tile_audio=False, **off)
        assert ab.single_view(AB.CLIPS[kind, False](), True) == "out"
        assert list(ab._frontends) == [("config", True, rate)] and ab.log == AB.expected(AB.SINGLE[True, False, False], kind)
    assert [s[0] for s in ingests] == ["pcm_wave", "pcm_ingest"]
