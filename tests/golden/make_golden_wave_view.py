"""Fixture for the waveform views of the log-mel front-end (vipant_fbank_view / vipant_wave_view): what the REFERENCE's own
transform classes (cvap/data/audio/transform.py:75-202) and its pipeline crop (:24-26) make of seeded clips, stage by stage.

    python tests/golden/make_golden_wave_view.py /path/to/reference      # writes tests/golden/wave_view.npz (data only)

The reference's transform.py is loaded by file path with stub modules for the imports it does not need here (torchaudio,
torchvision.transforms, omegaconf).  Each stage is one call of the class's static method; the draw a method makes is recovered by
re-seeding np.random and repeating the call it makes (np.random.randint / uniform / rand), and stored the way the front-end takes
it: a window position `left` out of `range` as u = (left + 0.5) / range, a scale factor as the factor, a noise draw as its snr.
torch.normal is patched to record the standard deviation RandomNoise asks for and to return zeros, so the stored signals are the
noise-free ones and `sigma` is the reference's own figure.

Clips are 16-bit PCM (integers / 32768) at 16 kHz: tones plus noise under a three-segment amplitude envelope, which is what makes
the crop rule take the drawn window, the head or the tail.  Every comparison of standard deviations the rule makes on these clips
clears by a factor of at least 1.01 (asserted below, on a float64 restatement of the rule): near-ties legitimately depend on the
order of a floating-point sum.  Between them the cases hit all three outcomes, for the chain's crop and for the pipeline's.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SR, MAX_LEN = 16000, 64
L = int((MAX_LEN / 100 + 0.05) * SR)            # 11040
MARGIN = 1.01


def load_reference(root):
    def stub(name, **kw):
        m = types.ModuleType(name)
        m.__dict__.update(kw)
        sys.modules[name] = m

    class Anything:
        def __init__(self, *a, **k):
            pass
    stub("torchaudio")
    stub("torchaudio.transforms", FrequencyMasking=Anything, TimeMasking=Anything)
    stub("omegaconf")
    stub("omegaconf.listconfig", ListConfig=list)
    stub("omegaconf.dictconfig", DictConfig=dict)
    stub("torchvision")
    stub("torchvision.transforms", Compose=Anything, ToTensor=Anything, Normalize=Anything)
    spec = importlib.util.spec_from_file_location("reference_transform", os.path.join(root, "cvap", "data", "audio", "transform.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def clip(n, seed, envelope=((1.0, 0.1),)):
    """16-bit PCM: two tones + noise, scaled per segment: envelope = ((fraction of the clip, amplitude), ...)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    x = np.sin(2 * np.pi * (310.0 + 40.0 * seed) * t) + 0.5 * np.sin(2 * np.pi * 1733.0 * t + 1.0) + 0.5 * rng.standard_normal(n)
    amp, start = np.zeros(n), 0
    for frac, a in envelope:
        stop = min(n, start + int(round(frac * n)))
        amp[start:stop] = a
        start = stop
    amp[start:] = envelope[-1][1]
    pcm = np.clip(np.round(x * amp * 32768.0 + 37.0), -32768, 32767)          # (+37: a DC offset for the zero-mean to remove)
    return (pcm / 32768.0).astype(np.float32)


def std64(v):
    return float(np.std(np.asarray(v, dtype=np.float64), ddof=1))


def rule_outcome(x, left, length):
    """float64 restatement of RandomCrop.random_crop's decisions -> (outcome 0 window / 1 head / 2 tail, smallest margin)."""
    old, new = 0.5 * std64(x), std64(x[left:left + length])
    margins = [max(old, new) / min(old, new)]
    if not new < old:
        return 0, min(margins)
    head = std64(x[:length])
    margins.append(max(new, head) / min(new, head))
    return (2 if new > head else 1), min(margins)


class Runner:
    def __init__(self, ref):
        self.ref, self.sigma = ref, None

    def crop(self, x, length, train, seed):
        """-> (cropped, left of what was taken, u, outcome)"""
        n = x.shape[-1]
        if n <= length:
            return x, 0, 0.0, -1
        np.random.seed(seed)
        y = self.ref.RandomCrop.random_crop(x, length, train)
        if train:
            np.random.seed(seed)
            left = int(np.random.randint(0, n - length))
        else:
            left = int(round(0.5 * (n - length)))
        outcome, margin = rule_outcome(x[0].numpy(), left, length)
        assert margin >= MARGIN, ("near-tie in the crop rule", margin)
        taken = (left, 0, n - length)[outcome]
        assert torch.equal(y, x[..., taken:taken + length]), "the restated rule and the reference disagree"
        return y, taken, (left + 0.5) / (n - length), outcome

    def run(self, x0, chain, train, seed):
        """chain: dict of the stages' parameters; -> record of arrays / scalars"""
        ref, x = self.ref, torch.from_numpy(x0).unsqueeze(0)
        rec = {"x0": x0, "draws": np.array([0.0, 1.0, 0.0, 0.0, -1.0, 0.0]), "train": int(train)}
        if chain.get("flip"):
            x = ref.RandomFlip.random_flip(x, 1.0)                     # torch.rand(1) <= 1.0: always
            rec["draws"][0] = 1.0
        if "scale" in chain:
            np.random.seed(seed + 1)
            x = ref.RandomScale.random_scale(x, chain["scale"], False)
            np.random.seed(seed + 1)
            rec["draws"][1] = float(np.power(chain["scale"], np.random.uniform(-1, 1)))
        rec["n2"] = x.shape[-1]
        if "pad" in chain and x.shape[-1] < chain["pad"]:
            n = x.shape[-1]
            np.random.seed(seed + 2)
            x = ref.RandomPad.random_pad(x, chain["pad"], True, chain.get("padding_value"))
            np.random.seed(seed + 2)
            left = int(np.random.randint(0, chain["pad"] - n))
            rec["draws"][2], rec["pad_left"] = (left + 0.5) / (chain["pad"] - n), left
        rec["n3"] = x.shape[-1]
        rec["crop_left"] = rec["crop_outcome"] = -1
        if "crop" in chain:
            x, rec["crop_left"], rec["draws"][3], rec["crop_outcome"] = self.crop(x, chain["crop"], True, seed + 3)
        rec["n4"] = x.shape[-1]
        rec["sigma"] = 0.0
        if "snr" in chain:
            lo, hi = chain["snr"]
            np.random.seed(seed + 4)
            y = ref.RandomNoise.random_noise(x, lo, hi, 1.0)           # np.random.rand() > 1.0: never skipped
            np.random.seed(seed + 4)
            np.random.rand()
            rec["draws"][4] = float(np.random.rand() * (hi - lo + 1.0) + lo)
            assert torch.equal(y, x)                                   # (the patched torch.normal returned zeros)
            rec["sigma"] = float(self.sigma)
        x, rec["final_left"], rec["draws"][5], rec["final_outcome"] = self.crop(x, L, train, seed + 5)
        rec["out"] = x[0].numpy().copy()
        return rec


def main():
    ref = load_reference(sys.argv[1])
    run = Runner(ref)
    real_normal = torch.normal

    def fake_normal(mean, std, shape):
        run.sigma = float(std)
        return torch.zeros(shape)
    torch.normal = fake_normal
    quiet_head = ((0.15, 0.001), (0.60, 0.02), (0.25, 1.0))            # ultra-quiet start, quiet middle, loud ending -> the tail
    loud_head = ((0.35, 0.5), (0.65, 0.01))                            # loud start, quiet rest -> the head
    clips = {
        "a4000": clip(4000, 1), "a11040": clip(11040, 2), "a11041": clip(11041, 3), "a20000": clip(20000, 4),
        "head20000": clip(20000, 5, loud_head), "tail20000": clip(20000, 6, quiet_head), "zero4000": np.zeros(4000, np.float32),
        "q4000": clip(4000, 7, ((1.0, 0.05),)), "q20000": clip(20000, 8, ((1.0, 0.05),)),
    }
    full = {"flip": True, "scale": 1.5, "pad": 12000, "crop": 11500}
    cases = [   # name, clip, chain, train, seed
        ("flip_4000", "a4000", {"flip": True}, True, 10),
        ("flip_20000", "a20000", {"flip": True}, True, 11),
        ("scale_4000_a", "a4000", {"scale": 1.5}, True, 12),
        ("scale_4000_b", "a4000", {"scale": 1.5}, True, 15),
        ("scale_11041", "a11041", {"scale": 1.5}, True, 14),
        ("pad_4000", "a4000", {"pad": 8000}, True, 20),
        ("pad_4000_value", "a4000", {"pad": 8000, "padding_value": 0.25}, True, 21),
        ("crop_window", "a20000", {"crop": 6000}, True, 30),
        ("crop_head", "head20000", {"crop": 6000}, True, 31),
        ("crop_tail", "tail20000", {"crop": 6000}, True, 32),
        ("final_11040_eval", "a11040", {}, False, 40),
        ("final_11041_train", "a11041", {}, True, 41),
        ("final_11041_eval", "a11041", {}, False, 42),
        ("final_window_eval", "a20000", {}, False, 43),
        ("final_head_train", "head20000", {}, True, 48),
        ("final_tail_eval", "tail20000", {}, False, 45),
        ("final_tail_train", "tail20000", {}, True, 46),
        ("noise_4000", "q4000", {"snr": (10.0, 20.0)}, True, 50),
        ("noise_20000", "q20000", {"snr": (10.0, 20.0)}, True, 51),
        ("noise_zero", "zero4000", {"snr": (10.0, 120.0)}, True, 52),
        ("chain_4000", "a4000", dict(full), True, 60),
        ("chain_20000", "tail20000", dict(full), True, 61),
        ("chain_11041_noise", "a11041", dict(full, snr=(100.0, 110.0)), True, 62),
    ]
    out = {"clip/" + k: v for k, v in clips.items()}
    out["meta/sample_rate"], out["meta/max_len"], out["meta/final_len"] = np.array(SR), np.array(MAX_LEN), np.array(L)
    names, outcomes = [], {"crop": set(), "final": set()}
    for name, cname, chain, train, seed in cases:
        rec = run.run(clips[cname], chain, train, seed)
        names.append(name)
        out[f"case/{name}/clip"] = np.array(cname)
        out[f"case/{name}/chain"] = np.array([float(bool(chain.get("flip"))), float(chain.get("scale", 0.0)), float(chain.get("pad", 0)),
                                              float(chain.get("crop", 0)), *chain.get("snr", (-1.0, -1.0)),
                                              float(chain.get("padding_value", np.nan))])
        for k in ("draws", "train", "n2", "n3", "n4", "crop_left", "crop_outcome", "final_left", "final_outcome", "sigma"):
            out[f"case/{name}/{k}"] = np.array(rec[k])
        out[f"case/{name}/pad_left"] = np.array(rec.get("pad_left", 0))
        start = max(int(rec["crop_left"]), 0) + int(rec["final_left"])
        if np.array_equal(rec["out"], rec["x0"][start:start + rec["out"].shape[0]]):      # a plain window of the clip is stored as its start
            out[f"case/{name}/out_start"], out[f"case/{name}/out_len"] = np.array(start), np.array(rec["out"].shape[0])
        else:
            out[f"case/{name}/out"] = rec["out"]
        outcomes["crop"].add(int(rec["crop_outcome"]))
        outcomes["final"].add(int(rec["final_outcome"]))
        print(f"{name:20s} n0 {rec['x0'].shape[0]:6d} n2 {rec['n2']:6d} n3 {rec['n3']:6d} n4 {rec['n4']:6d} crop {rec['crop_left']:6d}/"
              f"{rec['crop_outcome']:2d} final {rec['final_left']:6d}/{rec['final_outcome']:2d} out {rec['out'].shape[0]:6d} sigma {rec['sigma']:.6g} "
              f"draws {np.round(rec['draws'], 4).tolist()}")
    torch.normal = real_normal
    assert {0, 1, 2} <= outcomes["crop"] and {0, 1, 2} <= outcomes["final"], outcomes
    assert int(out["case/final_11041_train/final_left"]) == 0
    assert abs(float(out["case/noise_zero/sigma"]) - 1e-7 ** 0.5) < 1e-9             # a silent clip: the 1e-7 floor alone
    out["meta/cases"] = np.array(names)
    path = os.path.join(HERE, "wave_view.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
