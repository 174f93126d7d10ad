"""vipant_image_view on the device against PIL's bytes (tests/golden/image_view.npz) and the fp64 restatement
(tests/image_view_ref.py).  Normalisation "off" is mean 0, std 1: the output is then code / 255 in fp32.

Bounds, and where they come from:
  * resample, crop, flip, `clip`, gray and solarise from uint8 input: bit contracts (integer arithmetic; L of integers is exact in fp32);
  * brightness / contrast / saturation from uint8 input: floor(255 out) is PIL's wherever the restated value is not within 1e-3 of an
    integer; values the clip put on 0 or 255 are exact and stay in the comparison; at most 2 % of the values may be left out;
  * a float stage against the restatement: 1e-3 code values (about 50 fp32 roundings of 255 * 2^-24, the longest stage being the six
    blur passes); a whole chain: 5e-3 (the jitter factors amplify by at most 1.4^3).  Left out are the pixels the restatement flags
    as within 1e-2 of a gray rounding tie or of the solarise threshold (through a blur: everything such a pixel reaches), at most
    2 % of an image.  The rows of the whole-chain test are drawn by `draw_image_views`; a row whose image the RESTATEMENT flags beyond
    2 % is passed over (a frame of few colours keeps that rare for the prime view; behind the second view's certain blur a single tie
    spreads over a 7 x 7 to 13 x 13 neighbourhood) -- the selection never looks at the kernel;
  * hue and blur against PIL (which quantises in HSV and between its box passes): the kernel's mean distance to PIL is at most 1.5 x
    the restatement's own, computed here."""
import numpy as np
import pytest
import torch

import image_view_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MEAN, STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
OFF = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
N = 32


@pytest.fixture(scope="module")
def fx(golden):
    return golden("image_view")


@pytest.fixture(scope="module")
def frames():
    return {name: ref.seeded_frame(h, w, seed, noise) for name, (h, w, seed, noise, n) in ref.CLIP_CASES.items()}


def views(chain="barlow", norm=OFF, n=N, which="prime"):
    from vipant_amd.image_views import ImageViews
    return ImageViews(n, chain, norm[0], norm[1], device=DEV, which=which)


def dev(frame):
    return torch.from_numpy(np.ascontiguousarray(frame)).unsqueeze(0).to(DEV)


def want(codes, norm=OFF):
    """((v / 255) - mean) / std evaluated by torch in fp32, [n, n, 3] codes -> [3, n, n]"""
    v = torch.from_numpy(np.ascontiguousarray(codes)).to(torch.float32).permute(2, 0, 1)
    m, s = (torch.tensor(t, dtype=torch.float32).view(3, 1, 1) for t in norm)
    return ((v / 255.0) - m) / s


def codes_of(out):
    """normalisation off: fp32 [3, n, n] -> fp64 code values [n, n, 3]"""
    return out.detach().cpu().double().permute(1, 2, 0).numpy() * 255.0


def run_row(frame, row, flags=ref.ALL, norm=OFF, n=N):
    return views(norm=norm, n=n)(dev(frame), draws=torch.from_numpy(np.asarray(row)[None]), chain_flags=flags)[0]


def padded(batch, fill, hmax, wmax):
    buf = np.full((len(batch), hmax, wmax, 3), fill, dtype=np.uint8)
    for i, f in enumerate(batch):
        buf[i, :f.shape[0], :f.shape[1]] = f
    return torch.from_numpy(buf).to(DEV), torch.tensor([[f.shape[0], f.shape[1]] for f in batch], dtype=torch.int32)


def test_clip_end_to_end_is_pil_bit_for_bit(fx, frames):
    small = [k for k, c in ref.CLIP_CASES.items() if c[4] == N]
    singles = {}
    for norm in (OFF, (MEAN, STD)):
        for name in ref.CLIP_CASES:
            n = ref.CLIP_CASES[name][4]
            out = views("clip", norm, n)(dev(frames[name]))
            assert out.shape == (1, 3, n, n) and out.dtype == torch.float32
            assert torch.equal(out[0].cpu(), want(fx["clip_" + name], norm)), (name, norm)
            singles[(name, norm)] = out[0]
    assert torch.equal(singles[("32x32", OFF)].cpu(), want(frames["32x32"]))             # the identity returns its input
    # one batch of every small case inside a larger buffer whose padding is poison: the same bits as the singles, for both poisons
    for fill in (255, 0):
        buf, hw = padded([frames[k] for k in small], fill, 260, 258)
        out = views("clip", (MEAN, STD))(buf, hw)
        for i, k in enumerate(small):
            assert torch.equal(out[i], singles[(k, (MEAN, STD))]), (k, fill)
        assert bool((buf.cpu() == padded([frames[k] for k in small], fill, 260, 258)[0].cpu()).all())
    # a non-contiguous view of a wider buffer (strides passed through)
    buf, hw = padded([frames["37x53"]], 7, 64, 128)
    assert torch.equal(views("clip", (MEAN, STD))(buf[:, :50, 0:64], hw)[0], singles[("37x53", (MEAN, STD))])


def test_boxes_flip_and_rows_that_fire_nothing(fx, frames):
    for key, (fname, box) in ref.BOX_CASES.items():
        for norm in (OFF, (MEAN, STD)):
            out = run_row(frames[fname], ref.make_row(box), norm=norm)
            assert torch.equal(out.cpu(), want(fx["box_" + key], norm)), key                      # exactly the resample of its box
            flipped = run_row(frames[fname], ref.make_row(box, flip=1), norm=norm)
            assert torch.equal(flipped, out.flip(-1)), key
            assert torch.equal(run_row(frames[fname], ref.make_row(box, flip=1), flags=ref.ALL & ~ref.FLIP, norm=norm), out)
    # the full-frame box of a square frame is the clip chain; stages the chain flags switch off do not run
    f = frames["32x32"]
    full = ref.make_row((0, 0, 32, 32))
    assert torch.equal(run_row(f, full, norm=(MEAN, STD)), views("clip", (MEAN, STD))(dev(f))[0])
    busy = ref.make_row((0, 0, 32, 32), order=(0, 1, 2, 3), factors=(0.7, 1.3, 0.9, 0.05), gray_on=1, sigma=1.0, solar=1)
    assert torch.equal(run_row(f, busy, flags=ref.FLIP, norm=(MEAN, STD)), views("clip", (MEAN, STD))(dev(f))[0])
    neutral = ref.make_row((0, 0, 32, 32), order=(3, 2, 1, 0))
    assert torch.equal(run_row(f, neutral, norm=(MEAN, STD)), views("clip", (MEAN, STD))(dev(f))[0])       # neutral factors: untouched


def _bases(fx):
    return {"noise": (fx["frame_48x64"], (8, 16, 32, 32)), "smooth": (fx["base_smooth"], (0, 0, 32, 32))}


def test_gray_and_solarise_from_uint8_are_exact(fx):
    for tag, (frame, box) in _bases(fx).items():
        assert torch.equal(run_row(frame, ref.make_row(box)).cpu(), want(fx["base_" + tag]))      # the stage input is PIL's input
        g = np.repeat(fx["gray_" + tag][..., None], 3, axis=-1)
        for norm in (OFF, (MEAN, STD)):
            assert torch.equal(run_row(frame, ref.make_row(box, gray_on=1), norm=norm).cpu(), want(g, norm)), tag
            assert torch.equal(run_row(frame, ref.make_row(box, solar=1), norm=norm).cpu(), want(fx["solar_" + tag], norm)), tag


def test_brightness_contrast_saturation_from_uint8_floor_to_pil(fx):
    stages = (("bright", 0, ref.brightness), ("contrast", 1, ref.contrast), ("color", 2, lambda x, a: ref.saturation(x, a)[0]))
    for tag, (frame, box) in _bases(fx).items():
        base = fx["base_" + tag].astype(np.float64)
        for name, op, fn in stages:
            masked = total = 0
            for i, f in enumerate(fx["factors"]):
                fac = [1.0, 1.0, 1.0, 0.0]
                fac[op] = float(f)
                got = codes_of(run_row(frame, ref.make_row(box, order=(op, (op + 1) % 4, (op + 2) % 4, (op + 3) % 4), factors=fac)))
                v = fn(base, float(np.float32(f)))
                fr = v - np.floor(v)
                keep = (np.minimum(fr, 1.0 - fr) > 1e-3) | (v == 0.0) | (v == 255.0)
                bad = int((np.floor(got) != fx[f"{name}_{tag}"][i])[keep].sum())
                print(f"{tag} {name} {f}: masked {1 - keep.mean():.4f} mismatches {bad} max |kernel - restatement| {np.abs(got - v).max():.2e}")
                assert bad == 0, (tag, name, f)
                masked, total = masked + int((~keep).sum()), total + keep.size
            assert masked <= 0.02 * total, (tag, name, masked / total)
        deg = run_row(frame, ref.make_row(box, order=(1, 0, 2, 3), factors=(1.0, 0.0, 1.0, 0.0)))      # factor 0: the degenerate image
        assert torch.equal(deg.cpu(), want(np.full((N, N, 3), fx["contrast_deg_" + tag], dtype=np.uint8))), tag      # ... is PIL's
        assert abs(ref.contrast_mean(base)[1] + 0.5 - round(ref.contrast_mean(base)[1] + 0.5)) > 0.01


def _check(got, x, near, tol, what):
    err = np.abs(got - x).max(axis=-1)
    share = float(near.mean())
    worst = float(err[~near].max()) if (~near).any() else 0.0
    print(f"{what}: max error {worst:.2e} code values, {share:.4f} of the pixels left out")
    assert share <= 0.02, (what, share)
    assert worst <= tol, (what, worst)


def test_float_stages_against_the_restatement(fx):
    """Each stage on float input: a brightness of 0.77 in front of it turns the uint8 codes into non-integers."""
    noise, blocks = (fx["frame_48x64"], (8, 16, 32, 32)), (fx["blocks32"], (0, 0, 32, 32))
    cases = [("contrast", noise, dict(order=(0, 1, 2, 3), factors=(0.77, 1.31, 1.0, 0.0))),
             ("hue", noise, dict(order=(0, 3, 1, 2), factors=(0.77, 1.0, 1.0, 0.083))),
             ("hue-", noise, dict(order=(0, 3, 1, 2), factors=(0.77, 1.0, 1.0, -0.1))),
             ("saturation", blocks, dict(order=(0, 2, 1, 3), factors=(0.77, 1.0, 1.19, 0.0))),
             ("saturation-", blocks, dict(order=(0, 2, 1, 3), factors=(0.77, 1.0, 0.8, 0.0))),
             ("gray", blocks, dict(order=(0, 1, 2, 3), factors=(0.77, 1.0, 1.0, 0.0), gray_on=1)),
             ("solarise", noise, dict(order=(0, 1, 2, 3), factors=(1.23, 1.0, 1.0, 0.0), solar=1)),
             ("brightness", noise, dict(order=(0, 1, 2, 3), factors=(1.387, 1.0, 1.0, 0.0)))]
    cases += [(f"blur {s}", noise, dict(order=(0, 1, 2, 3), factors=(0.77, 1.0, 1.0, 0.0), sigma=s)) for s in (0.1, 0.7, 1.3, 2.0, 3.7)]
    for what, (frame, box), kw in cases:
        row = ref.make_row(box, **kw)
        x, near, means = ref.view(frame, row, N)
        for m in means:
            assert abs(m + 0.5 - round(m + 0.5)) > 0.01, (what, m)                     # the contrast mean is not near a tie
        _check(codes_of(run_row(frame, row)), x, near, 1e-3, what)


def _fired(row):
    return {name for name, on in (("jitter", row[ref.D_ORD0] >= 0), ("gray", row[ref.D_GRAY] > 0), ("blur", row[ref.D_SIGMA] > 0),
                                  ("solarise", row[ref.D_SOLAR] > 0), ("flip", row[ref.D_FLIP] > 0)) if on}


def _chain_rows(which, frame, count=8):
    """Rows from draw_image_views, seeds 0, 1, ... in order.  A row is kept when the restatement flags at most 2 % of its image; after
    `count` rows only those that fire a stage no kept row has fired yet, until every stage of the view has fired."""
    iv = views(which=which)
    need = {"jitter", "gray", "blur", "flip"} | ({"solarise"} if which == "prime" else set())
    rows, seen = [], set()
    for seed in range(400):
        for row in iv.draw_image_views([list(frame.shape[:2])] * 6, torch.Generator().manual_seed(seed)).numpy():
            if len(rows) >= count and not (_fired(row) - seen):
                continue
            x, near, means = ref.view(frame, row, N)
            if near.mean() <= 0.02 and all(abs(m + 0.5 - round(m + 0.5)) > 0.01 for m in means):
                rows.append((row, x, near))
                seen |= _fired(row)
            if len(rows) >= count and need <= seen:
                return rows
    raise AssertionError(f"no rows found for {need - seen}")


@pytest.mark.parametrize("which", ["prime", "second"])
def test_whole_chains_against_the_restatement(which):
    frame = ref.block_frame(64, 34, 16)[:48]
    rows = _chain_rows(which, frame)
    d = np.stack([r[0] for r in rows])
    print(which, len(rows), "rows; fired:", sorted(set().union(*[_fired(r) for r in d])))
    buf = torch.from_numpy(np.stack([frame] * len(rows))).to(DEV)
    out = views(which=which)(buf, draws=torch.from_numpy(d))
    for i, (row, x, near) in enumerate(rows):
        _check(codes_of(out[i]), x, near, 5e-3, f"{which} row {i}")
    again = views(which=which)(buf, draws=torch.from_numpy(d))
    assert torch.equal(out, again)                                                      # two runs, equal bits
    for i in range(len(rows)):                                                          # a batch is its items run singly
        assert torch.equal(views(which=which)(buf[i:i + 1], draws=torch.from_numpy(d[i:i + 1]))[0], out[i]), i
    normed = views(norm=(MEAN, STD), which=which)(buf, draws=torch.from_numpy(d))
    m, s = (torch.tensor(t, device=DEV).view(1, 3, 1, 1) for t in (MEAN, STD))
    assert torch.allclose(normed * s + m, out, atol=1e-6)


def test_hue_and_blur_are_no_further_from_pil_than_the_restatement(fx):
    for tag, (frame, box) in _bases(fx).items():
        base = fx["base_" + tag].astype(np.float64)
        for kind, params in (("hue", fx["hues"]), ("blur", fx["sigmas"])):
            for i, p in enumerate(params):
                if kind == "hue":
                    row, x = ref.make_row(box, order=(3, 0, 1, 2), factors=(1.0, 1.0, 1.0, float(p))), ref.hue(base, float(np.float32(p)))
                else:
                    row, x = ref.make_row(box, sigma=float(p)), ref.blur(base, float(p))
                got, pil = codes_of(run_row(frame, row)), fx[f"{kind}_{tag}"][i].astype(np.float64)
                dk, dr = np.abs(got - pil), np.abs(x - pil)
                print(f"{tag} {kind} {float(p):+.3f}: kernel to PIL mean {dk.mean():.3f} max {dk.max():.2f}; restatement to PIL mean "
                      f"{dr.mean():.3f} max {dr.max():.2f}; kernel to restatement max {np.abs(got - x).max():.2e}")
                assert dk.mean() <= 1.5 * dr.mean(), (tag, kind, p)


def test_sentinels_refusals_and_dtypes(frames):
    from vipant_amd._ffi import VipantError
    iv = views(norm=(MEAN, STD))
    f = frames["37x53"]
    rows = np.stack([ref.make_row((3, 5, 29, 41), flip=1, order=(2, 0, 3, 1), factors=(0.8, 1.2, 1.1, -0.05), gray_on=0, sigma=1.1, solar=1),
                     ref.make_row((0, 0, 37, 53))])
    buf = torch.from_numpy(np.stack([f, f])).to(DEV)
    plain = iv(buf, draws=torch.from_numpy(rows))
    ring = torch.full((2 * 3 * N * N + 512,), -777.0, device=DEV)
    out = ring[256:256 + 2 * 3 * N * N].view(2, 3, N, N)
    assert iv(buf, draws=torch.from_numpy(rows), out=out) is out
    assert torch.equal(out, plain) and bool((ring[:256] == -777.0).all()) and bool((ring[-256:] == -777.0).all())
    # refusals: nothing is written
    ring.fill_(-777.0)
    inside, outside = ref.seeded_frame(256, 256, 1, 96), ref.seeded_frame(257, 257, 1, 96)
    views("clip")(dev(inside))                                                          # just inside the downscale limit: served
    bad_rows = [ref.make_row((0, 0, 38, 53)), ref.make_row((-1, 0, 10, 10)), ref.make_row((0, 0, 0, 10)), ref.make_row((0.5, 0, 10, 10)),
                ref.make_row((0, 0, 37, 53), order=(0, 0, 1, 2))]
    for row in bad_rows:
        with pytest.raises(VipantError, match="code -1"):
            iv(buf, draws=torch.from_numpy(np.stack([rows[1], row])), out=out)
    with pytest.raises(VipantError, match="downscale limit"):
        views("clip")(dev(outside), out=out[:1])
    with pytest.raises(VipantError, match="downscale limit"):
        iv(dev(outside), draws=torch.from_numpy(ref.make_row((0, 0, 257, 257))[None]), out=out[:1])
    with pytest.raises(VipantError, match="code -1"):
        iv(buf, hw=torch.tensor([[37, 53], [0, 53]]), draws=torch.from_numpy(rows), out=out)
    with pytest.raises(VipantError, match="code -1"):
        iv(buf, hw=torch.tensor([[37, 53], [38, 53]]), draws=torch.from_numpy(rows), out=out)
    with pytest.raises(VipantError, match="uint8"):
        iv(buf.float(), draws=torch.from_numpy(rows))
    with pytest.raises(VipantError, match="no CPU path"):
        iv(buf.cpu(), draws=torch.from_numpy(rows))
    with pytest.raises(VipantError, match="needs draws"):
        iv(buf)
    torch.cuda.synchronize()
    assert bool((ring == -777.0).all())
    assert torch.equal(iv(buf, draws=torch.from_numpy(rows)), plain)                     # and the next call is served as before
