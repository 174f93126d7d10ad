"""The waveform views of the log-mel front-end (vipant_fbank_view / vipant_wave_view; KaldiFbank(..., view=), view_wave) against
tests/golden/wave_view.npz: what the reference's own transform classes and its pipeline crop (cvap/data/audio/transform.py:75-202,
:24-26) make of seeded clips, recorded by tests/golden/make_golden_wave_view.py.  sample_rate 16000, max_len 64 (final length
L = 11040), 512-point transforms; clips of 4000 (shorter than every target), 11040 (exactly L), 11041 (a crop by one sample) and
20000 samples (a real crop).

Bounds.  Flip, pad and crop copy samples: bit for bit.  RandomScale blends two samples with bit-equal indices and weights; its
three roundings may be contracted (the kernel pins one product and one fused multiply-add), which moves a sample by at most
2^-22 max|x| of its clip.  The noise z is compared with a float64 restatement of the Philox4x32-10 / Box-Muller recipe (below, with
its known-answer check) within 1e-5: logf <= 2 ulp, sqrtf 1/2 ulp, cospif <= 2 ulp, the product 1/2 ulp: 5 x 2^-24 x 5.8 = 1.7e-6,
times about 6 for the fp32 chain behind the reference's sigma; the noise cases use quiet clips and low snr so that the rounding of
x + sigma z itself (half an ulp of |x| <= 0.25, over sigma >= 4e-3: 4e-6) stays inside that.  Observed: profiles/wave_view_observed.txt.
The filter-bank bounds are tests/test_fbank_mix_gpu.py's for the same comparison (max 2e-3, mean 5e-5 without norms) plus the
oracle's own distance between the fixture's waveform and a float64 restatement of the blend on these clips, computed here."""
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
SR, MAX_LEN, F, L = 16000, 64, 128, 11040
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wave_view.npz")
PLAN_WORDS = ("n0", "n2", "n3", "n4", "n_out", "flags", "pad_left", "crop_left", "final_left")     # include/vipant_hip.h: the plan's first words


# ------------------------------------------------------------------ the fixture
@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    assert int(z["meta/final_len"]) == L and int(z["meta/sample_rate"]) == SR and int(z["meta/max_len"]) == MAX_LEN
    cases = {}
    for name in z["meta/cases"].tolist():
        c = {k: z[f"case/{name}/{k}"] for k in ("chain", "draws", "train", "n2", "n3", "n4", "crop_left", "crop_outcome", "final_left",
                                                 "final_outcome", "sigma", "pad_left")}
        c["x0"] = z["clip/" + str(z[f"case/{name}/clip"])]
        if f"case/{name}/out" in z.files:
            c["out"] = z[f"case/{name}/out"]
        else:
            s, n = int(z[f"case/{name}/out_start"]), int(z[f"case/{name}/out_len"])
            c["out"] = c["x0"][s:s + n]
        cases[name] = c
    return cases


def chain_of(c):
    flip, scale, pad, crop, lo, hi, value = c["chain"].tolist()
    chain = []
    if flip:
        chain.append(["RandomFlip", [1.0]])
    if scale:
        chain.append(["RandomScale", [scale]])
    if pad:
        chain.append(["RandomPad", {"output_len": int(pad), "padding_value": None if np.isnan(value) else value}])
    if crop:
        chain.append(["RandomCrop", [int(crop)]])
    if lo >= 0:
        chain.append(["RandomNoise", [lo, hi, 1.0]])
    return chain


def frontend(chain=(), train=True, zero_mean_wf=False, max_len=MAX_LEN, **kw):
    from vipant_amd.frontend import KaldiFbank
    return KaldiFbank(SR, F, max_len, zero_mean_wf=zero_mean_wf, audio_transforms=chain, train=train, device=DEV, **kw)


def plans(b):
    """The per-clip plans the last view call left in the front-end's workspace -> {field: [b] int}."""
    from vipant_amd import _ffi, ops
    ws = ops.scratch("fbank", _ffi.query("vipant_fbank_view_workspace_bytes", b), torch.device(DEV))
    words = ws[:b * 64].view(torch.int32).view(b, 16).cpu()
    return {k: words[:, i].tolist() for i, k in enumerate(PLAN_WORDS)}


SEED = 0x1234ABCD5678


@functools.lru_cache(maxsize=None)
def run_case(name, zero_mean_wf=False):
    """One fixture case through view_wave, as row 0 of a batch of two (row 1: an untouched short clip) -> (wave [n], plan of row 0)."""
    c = golden()[name]
    fb = frontend(chain_of(c), bool(c["train"]), zero_mean_wf)
    n0 = c["x0"].shape[0]
    wave = torch.zeros(2, n0)
    wave[0] = torch.from_numpy(c["x0"])
    wave[1, :1000] = 0.1
    draws = torch.tensor([c["draws"].tolist(), [0.0, 1.0, 0.0, 0.0, -1.0, 0.0]], dtype=torch.float64)
    out, nout = fb.view_wave(wave.to(DEV), torch.tensor([n0, 1000]).to(DEV), (draws, SEED))
    p = plans(2)
    out, nout = out.cpu(), nout.cpu()
    pad, crop = int(c["chain"][2]), int(c["chain"][3])
    assert out.shape == (2, L) and int(nout[1]) == min(max(1000, pad), crop or L, L)           # (a pad stage pads row 1 too)
    assert bool((out[0, int(nout[0]):] == 0).all()) and bool((out[1, int(nout[1]):] == 0).all())
    return out[0, :int(nout[0])].numpy(), {k: v[0] for k, v in p.items()}


def check_decisions(name, plan):
    c = golden()[name]
    for k in ("n2", "n3", "n4", "pad_left", "final_left"):
        assert plan[k] == int(c[k]), (name, k, plan[k], int(c[k]))
    if int(c["crop_left"]) >= 0:
        assert plan["crop_left"] == int(c["crop_left"]), (name, plan["crop_left"], int(c["crop_left"]))


# ------------------------------------------------------------------ the noise recipe, restated in float64
M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [n, 4], key (k0, k1) -> [n, 4] uint64 holding 32-bit words."""
    c = [np.asarray(counter[:, i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack(c, axis=1)


def normal64(seed, clip, k):
    k = np.asarray(k, dtype=np.uint64)
    counter = np.zeros((k.shape[0], 4), dtype=np.uint64)
    counter[:, 0] = k >> np.uint64(2)
    words = philox4x32_10(counter, (seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ clip))
    second = (k & np.uint64(2)) != 0
    wu, wv = np.where(second, words[:, 2], words[:, 0]), np.where(second, words[:, 3], words[:, 1])
    u = ((wu >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    v = ((wv >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    rad = np.sqrt(-2.0 * np.log(u))
    return rad * np.where((k & np.uint64(1)) != 0, np.sin(2.0 * np.pi * v), np.cos(2.0 * np.pi * v))


def test_philox_restatement_known_answer():
    got = philox4x32_10(np.zeros((1, 4), dtype=np.uint64), (0, 0))[0].tolist()
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [hex(int(w)) for w in got]


# ------------------------------------------------------------------ 1. stage by stage and the whole chain
COPIES = ["flip_4000", "flip_20000", "pad_4000", "pad_4000_value", "crop_window", "crop_head", "crop_tail", "final_11040_eval",
          "final_11041_train", "final_11041_eval", "final_window_eval", "final_head_train", "final_tail_eval", "final_tail_train"]
BLENDS = ["scale_4000_a", "scale_4000_b", "scale_11041", "chain_4000", "chain_20000"]


@pytest.mark.parametrize("name", COPIES)
def test_copy_stages_match_the_reference_bit_for_bit(name):
    c = golden()[name]
    got, plan = run_case(name)
    check_decisions(name, plan)
    assert got.shape == c["out"].shape, (got.shape, c["out"].shape)
    assert np.array_equal(got.view(np.int32), c["out"].view(np.int32))


def test_the_fixture_covers_every_outcome_of_the_crop_rule():
    g = golden()
    assert {int(g[n]["crop_outcome"]) for n in ("crop_window", "crop_head", "crop_tail")} == {0, 1, 2}
    assert {int(g[n]["final_outcome"]) for n in ("final_window_eval", "final_head_train", "final_tail_eval")} == {0, 1, 2}
    assert int(g["final_11041_train"]["final_left"]) == 0 and g["final_11041_train"]["out"].shape[0] == L


@pytest.mark.parametrize("name", BLENDS)
def test_scale_and_the_full_chain_match_within_the_blend_rounding(name):
    c = golden()[name]
    got, plan = run_case(name)
    check_decisions(name, plan)
    assert got.shape == c["out"].shape, (got.shape, c["out"].shape)
    err, bound = float(np.abs(got.astype(np.float64) - c["out"]).max()), 2.0 ** -22 * float(np.abs(c["x0"]).max())
    print(f"{name}: max |diff| {err:.3e} bound {bound:.3e}")
    assert err <= bound, (name, err, bound)


def test_full_chain_with_noise_keeps_its_decisions():
    """The noise fired (snr about 101 dB: the 1e-7 floor, sigma 3.2e-4): the decisions of the pipeline's crop, which sees the noisy
    signal, equal the reference's on its noise-free one, and what is left after taking sigma z away is the noise-free chain within
    the blend's rounding plus the noise bound (1e-5 sigma) plus the rounding of the sum (2^-24 max|x|)."""
    name = "chain_11041_noise"
    c = golden()[name]
    got, plan = run_case(name)
    check_decisions(name, plan)
    sigma = float(c["sigma"])
    k = np.arange(got.shape[0]) + plan["final_left"]
    rest = got.astype(np.float64) - sigma * normal64(SEED, 0, k)
    err = float(np.abs(rest - c["out"]).max())
    bound = (2.0 ** -22 + 2.0 ** -24) * float(np.abs(c["x0"]).max()) + 4e-5 * sigma        # 1e-5 sigma on z, and sigma itself to 6 x 2^-24 of 4.5 sigma
    print(f"{name}: max |noisy - sigma z - clean| {err:.3e} bound {bound:.3e}")
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------ 2. sigma and z together
@pytest.mark.parametrize("name", ["noise_4000", "noise_20000", "noise_zero"])
def test_noise_matches_the_restated_recipe(name):
    c = golden()[name]
    got, plan = run_case(name)
    check_decisions(name, plan)
    sigma = float(c["sigma"])
    if name == "noise_zero":
        assert abs(sigma - 1e-7 ** 0.5) < 1e-9 and not c["out"].any()
    z = (got.astype(np.float64) - c["out"]) / sigma
    want = normal64(SEED, 0, np.arange(got.shape[0]) + plan["final_left"])
    err = float(np.abs(z - want).max())
    print(f"{name}: sigma {sigma:.6g} max |z - restated| {err:.3e}")
    assert err < 1e-5, (name, err)


# ------------------------------------------------------------------ 3. noise hygiene
@functools.lru_cache(maxsize=None)
def pure_noise(seed):
    """z of three silent clips of 20000 samples (max_len 125: nothing is cropped) -> [3, 20000] float64."""
    fb = frontend([["RandomNoise", [10.0, 120.0, 1.0]]], True, False, max_len=125)
    draws = torch.tensor([[0.0, 1.0, 0.0, 0.0, 30.0, 0.0]] * 3, dtype=torch.float64)
    out, nout = fb.view_wave(torch.zeros(3, 20000, device=DEV), None, (draws, seed))
    assert nout.tolist() == [20000] * 3
    return out[:, :20000].cpu()


def test_noise_hygiene():
    n = 20000
    a, again, other = pure_noise(7), pure_noise.__wrapped__(7), pure_noise(8)
    assert torch.equal(a, again)                                               # a function of (seed, clip, index) alone
    sigma = float(np.float32(np.sqrt(np.float64(np.float32(1e-7)))))
    z, zo = a.double().numpy() / sigma, other.double().numpy() / sigma
    corr = lambda x, y: float(np.mean((x - x.mean()) * (y - y.mean())) / (x.std() * y.std()))
    for x, y, what in ((z[0], zo[0], "another seed"), (z[0], z[1], "another clip"), (z[1], z[2], "another clip")):
        assert abs(corr(x, y)) < 5 / np.sqrt(n), (what, corr(x, y))
    for i in range(3):
        assert abs(z[i].mean()) < 5 / np.sqrt(n), (i, z[i].mean())
        assert abs(z[i].var() - 1.0) < 5 * np.sqrt(2.0 / n), (i, z[i].var())
        for lag in (1, 2, 3, 4):                                               # a wrong counter or word mapping shows up here
            assert abs(corr(z[i][:-lag], z[i][lag:])) < 5 / np.sqrt(n), (i, lag)


# ------------------------------------------------------------------ 4. fused equals materialised
def mixed_batch():
    g = golden()
    lens = [4000, 11040, 11041, 20000, 20000]
    wave = torch.zeros(5, 20000)
    for i, name in enumerate(("flip_4000", "final_11040_eval", "final_11041_train", "final_tail_eval", "final_head_train")):
        wave[i, :lens[i]] = torch.from_numpy(g[name]["x0"])
    return wave.to(DEV), torch.tensor(lens).to(DEV)


FULL = [["RandomFlip", [0.5]], ["RandomScale", [1.5]], ["RandomPad", [12000]], ["RandomCrop", [11500]], ["RandomNoise", [10.0, 30.0, 0.6]]]


@pytest.mark.parametrize("frame_length,size", [(25.0, 512), (50.0, 1024), (100.0, 2048)])
@pytest.mark.parametrize("dressed", [False, True])
def test_fused_equals_materialised(frame_length, size, dressed):
    """fbank(view=) and vipant_fbank(zero_mean = 0) on view_wave()'s waveform: the same bits, with and without norms and masks."""
    kw = dict(frame_length=frame_length, norms=(-4.94, 5.76) if dressed else (), freq_mask_param=16 if dressed else 0,
              time_mask_param=20 if dressed else 0)
    fb, plain = frontend(FULL, True, True, **kw), frontend((), True, False, **kw)
    assert fb.padded == size
    wave, lens = mixed_batch()
    view = fb.draw_views(5, torch.Generator().manual_seed(size))
    assert bool((view[0][:, 0] == 1).any()) and bool((view[0][:, 4] >= 0).any()) and bool((view[0][:, 4] < 0).any())
    masks = fb.draw_masks(5, torch.Generator().manual_seed(3)) if dressed else None
    fused = fb(wave, lens, masks, view=view)
    mat, nout = fb.view_wave(wave, lens, view)
    assert nout.tolist() == [L] * 5                                            # padded to 12000, cropped to 11500, then to L
    assert abs(float(mat.double().mean(1).abs().max())) < 1e-6                 # zero_mean_wf happened inside the view
    want = plain(mat, nout, masks)
    assert torch.equal(fused, want)
    assert bool(torch.isfinite(fused).all())


# ------------------------------------------------------------------ 5. the identity plan
@pytest.mark.parametrize("train", [True, False])
def test_identity_view_keeps_the_bits_of_the_plain_launch(train):
    wave, lens = mixed_batch()
    wave, lens = wave[:3, :11040].contiguous(), torch.tensor([4000, 11040, 7777]).to(DEV)
    for kw in (dict(), dict(norms=(-4.94, 5.76), freq_mask_param=16, time_mask_param=20)):
        fb = frontend((), train, True, **kw)
        masks = fb.draw_masks(3, torch.Generator().manual_seed(5))
        assert torch.equal(fb(wave, lens, masks, view=True), fb(wave, lens, masks))
        assert torch.equal(fb(wave, lens, masks, view=fb.draw_views(3, torch.Generator().manual_seed(1))), fb(wave, lens, masks))


# ------------------------------------------------------------------ 6. against the CPU filter bank
def restated64(c):
    """The chain of one fixture case in float64 from its recorded draws and decisions (the blend unrounded)."""
    flip, scale, pad, crop, _, _, value = c["chain"].tolist()
    x = c["x0"].astype(np.float64)
    if flip:
        x = x[::-1]
    if scale:
        n1, n2, cf = x.shape[0], int(c["n2"]), np.float32(c["draws"][1])
        base = (np.arange(n2, dtype=np.float32) / cf).astype(np.float32)
        r1 = base.astype(np.int64)
        r2, r = np.minimum(r1 + 1, n1 - 1), (base - r1.astype(np.float32)).astype(np.float64)
        x = (1.0 - r) * x[r1] + r * x[r2]
    if pad and x.shape[0] < pad:
        left = int(c["pad_left"])
        lv, rv = (x[0], x[-1]) if np.isnan(value) else (value, value)
        x = np.concatenate([np.full(left, lv), x, np.full(int(pad) - left - x.shape[0], rv)])
    if crop and x.shape[0] > crop:
        x = x[int(c["crop_left"]):int(c["crop_left"]) + int(crop)]
    if x.shape[0] > L:
        x = x[int(c["final_left"]):int(c["final_left"]) + L]
    return x


@pytest.mark.parametrize("name", ["chain_4000", "chain_20000", "scale_11041", "crop_tail", "final_head_train", "pad_4000_value"])
def test_view_filter_bank_against_the_cpu_oracle(name):
    c = golden()[name]
    fb = frontend(chain_of(c), bool(c["train"]), True)
    n0 = c["x0"].shape[0]
    draws = torch.tensor([c["draws"].tolist()], dtype=torch.float64)
    got = fb(torch.from_numpy(c["x0"]).unsqueeze(0).to(DEV), torch.tensor([n0]).to(DEV), view=(draws, SEED)).cpu()[0, 0]
    ref = FB.spectrogram_item(torch.from_numpy(c["out"].copy()), SR, MAX_LEN, F, norms=(), zero_mean_wf=True)
    ref64 = FB.spectrogram_item(torch.from_numpy(restated64(c).astype(np.float32)), SR, MAX_LEN, F, norms=(), zero_mean_wf=True)
    own = (ref - ref64).abs()
    err = (got - ref).abs()
    print(f"{name}: max {float(err.max()):.3e} mean {float(err.mean()):.3e}; oracle's own distance max {float(own.max()):.3e} mean {float(own.mean()):.3e}")
    assert err.max() < 2e-3 + float(own.max()), (name, float(err.max()))
    assert err.mean() < 5e-5 + float(own.mean()), (name, float(err.mean()))


# ------------------------------------------------------------------ 7. clamps and refusals
def test_clamps_and_refusals():
    from vipant_amd import _ffi, ops
    g = golden()
    fb = frontend([["RandomScale", [1.5]], ["RandomPad", [12000]], ["RandomCrop", [11500]]], True, True)
    b, T = 3, MAX_LEN
    wave = torch.zeros(b, 20000)
    lens = [4000, 20000, 20000]
    for i, name in enumerate(("flip_4000", "final_window_eval", "final_tail_eval")):
        wave[i, :lens[i]] = torch.from_numpy(g[name]["x0"])
    wave, lens = wave.to(DEV), torch.tensor(lens).to(DEV)
    below = float(np.nextafter(1.0, 0.0))
    wild = torch.tensor([[0.0, 0.0, 1.5, -1.0, -1.0, 1.5], [0.0, -3.0, -1.0, 1.5, -1.0, -1.0], [0.0, float("nan"), 0.3, float("nan"), -1.0, 7.0]],
                        dtype=torch.float64)
    tame = torch.tensor([[0.0, 1.0, below, 0.0, -1.0, below], [0.0, 1.0, 0.0, below, -1.0, 0.0], [0.0, 1.0, 0.3, 0.0, -1.0, below]],
                        dtype=torch.float64)
    want = fb(wave, lens, view=(tame, 1))
    want_wave, want_n = fb.view_wave(wave, lens, (tame, 1))
    params, _ = fb._view_args((tame, 1), b, 20000, torch.device(DEV))
    nbytes = _ffi.query("vipant_fbank_view_workspace_bytes", b)
    assert nbytes == 256
    arena = torch.full((256 + nbytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)         # the workspace is exactly as large as asked
    ws_ptr = arena.data_ptr() + 256
    guard = 2 * T * F
    buf = torch.full((guard + b * T * F + guard,), -777.0, device=DEV)
    out_ptr = buf.data_ptr() + 4 * guard
    wbuf = torch.full((L + b * L + L,), -777.0, device=DEV)
    nbuf = torch.full((1 + b + 1,), -777, dtype=torch.int64, device=DEV)
    dw = wild.to(DEV)
    lib = _ffi.lib()

    def fbank_view(out=out_ptr, draws=dw.data_ptr(), nb=b, nt=T, p=params, ws=ws_ptr, wsb=nbytes, lens_ptr=lens.data_ptr()):
        return lib.vipant_fbank_view(wave.data_ptr(), 20000, lens_ptr, out, fb.window.data_ptr(), fb.banks.data_ptr(), fb.bank_start.data_ptr(),
                                     fb.bank_len.data_ptr(), None, nb, nt, F, fb.size, fb.shift, fb.padded, fb.preemphasis, 0.0, 0.0, p, draws,
                                     ws, wsb, ops._stream())

    def wave_view(out=wbuf.data_ptr() + 4 * L, nout=nbuf.data_ptr() + 8, draws=dw.data_ptr(), nb=b, stride=L, p=params):
        return lib.vipant_wave_view(wave.data_ptr(), 20000, lens.data_ptr(), out, stride, nout, nb, p, draws, ws_ptr, nbytes, ops._stream())

    bad = _ffi.ViewParams.from_buffer_copy(params)
    bad.final_len = 0
    bits = _ffi.ViewParams.from_buffer_copy(params)
    bits.stages = 1 << 5
    # refusals first: everything must still be all sentinel afterwards
    assert fbank_view(draws=None) != 0 and fbank_view(nb=0) != 0 and fbank_view(nt=0) != 0 and fbank_view(out=None) != 0
    assert fbank_view(p=bad) != 0 and fbank_view(p=bits) != 0 and fbank_view(ws=None) != 0 and fbank_view(wsb=nbytes - 1) != 0
    assert fbank_view(lens_ptr=None) != 0
    assert wave_view(draws=None) != 0 and wave_view(nb=0) != 0 and wave_view(out=None) != 0 and wave_view(nout=None) != 0
    assert wave_view(stride=0) != 0 and wave_view(p=bad) != 0
    assert "wave_view" in lib.vipant_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf == -777.0).all()) and bool((wbuf == -777.0).all()) and bool((nbuf == -777).all()) and bool((arena == 0xA5).all())
    assert fbank_view() == 0
    torch.cuda.synchronize()
    body = buf[guard:guard + b * T * F].view(b, T, F)
    assert bool(torch.isfinite(body).all())
    assert bool((buf[:guard] == -777.0).all()) and bool((buf[guard + b * T * F:] == -777.0).all())
    assert bool((arena[:256] == 0xA5).all()) and bool((arena[256 + nbytes:] == 0xA5).all())
    assert torch.equal(body, want[:, 0])                                       # a u of 1.5 / -1 / NaN and a scale <= 0: the clamped value's output
    assert wave_view() == 0
    torch.cuda.synchronize()
    assert torch.equal(wbuf[L:L + b * L].view(b, L), want_wave) and torch.equal(nbuf[1:1 + b], want_n)
    assert bool((wbuf[:L] == -777.0).all()) and bool((wbuf[L + b * L:] == -777.0).all()) and nbuf[0] == -777 and nbuf[-1] == -777
    assert bool((arena[:256] == 0xA5).all()) and bool((arena[256 + nbytes:] == 0xA5).all())
    with pytest.raises(_ffi.VipantError, match="exclude each other"):
        fb(wave, lens, mix=(torch.tensor([1, 0, -1], dtype=torch.int32), torch.ones(3)), view=True)
    with pytest.raises(_ffi.VipantError, match=r"\[3, 6\]"):
        fb(wave, lens, view=(tame[:2], 1))
