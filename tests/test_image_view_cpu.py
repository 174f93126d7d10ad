"""Image views without a GPU: the draw rules of `ImageViews.draw_image_views`, the restated resample (tests/image_view_ref.py) against
PIL's bytes in tests/golden/image_view.npz, chain selection from the config, the refusals that need no device, the ABI symbols and
the workspace query.  No PIL here: the fixture is PIL's word (tests/golden/make_golden_image_view.py wrote it)."""
import math
import os

import numpy as np
import pytest
import torch

import image_view_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("image_view")


def _views(chain="barlow", which="prime", n=32):
    from vipant_amd.image_views import ImageViews
    return ImageViews(n, chain, device="cpu", which=which)


def test_draws_follow_the_crop_rules_and_consume_a_fixed_number_of_uniforms():
    from vipant_amd import image_views as iv
    hw = [[37, 53], [360, 640], [48, 64], [5, 7], [1, 1], [200, 30], [30, 200]] * 40
    v = _views()
    g = torch.Generator().manual_seed(5)
    d = v.draw_image_views(hw, g)
    assert d.shape == (len(hw), 16) and d.dtype == torch.float64 and d.device.type == "cpu"
    after = torch.rand(3, generator=g, dtype=torch.float64)
    g2 = torch.Generator().manual_seed(5)
    torch.rand(len(hw), iv.UNIFORMS_PER_IMAGE, generator=g2, dtype=torch.float64)          # exactly this many, whatever fired
    assert torch.equal(after, torch.rand(3, generator=g2, dtype=torch.float64))
    assert torch.equal(d, v.draw_image_views(hw, torch.Generator().manual_seed(5)))          # the same seed, the same draws
    assert not torch.equal(d, v.draw_image_views(hw, torch.Generator().manual_seed(6)))
    for (H, W), row in zip(hw, d.tolist()):
        y0, x0, h, w = row[:4]
        assert all(float(x).is_integer() for x in row[:4])
        assert 0 <= y0 and 0 <= x0 and 1 <= h and 1 <= w and y0 + h <= H and x0 + w <= W                # the box is inside the frame
        central = (y0, x0) == ((H - h) // 2, (W - w) // 2)
        in_area = 0.08 * H * W - (h + w) <= h * w <= H * W + (h + w)                                   # (rounding of h and w)
        in_ratio = 3 / 4 * (1 - 1 / min(h, w)) - 1e-9 <= w / h <= 4 / 3 * (1 + 1 / min(h, w)) + 1e-9 if min(h, w) > 1 else True
        if not (in_area and in_ratio):                          # only the fallback may leave the bounds: central, clamped to the ratio
            assert central and (h == H or w == W)
        assert row[4] in (0.0, 1.0) and row[13] in (0.0, 1.0) and row[15] in (0.0, 1.0)
        if row[5] >= 0:
            assert sorted(row[5:9]) == [0.0, 1.0, 2.0, 3.0]
            assert 0.6 <= row[9] <= 1.4 and 0.6 <= row[10] <= 1.4 and 0.8 <= row[11] <= 1.2 and -0.1 <= row[12] <= 0.1
        else:
            assert row[5:13] == [-1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 0.0]
        assert row[14] == 0.0 or 0.1 <= row[14] <= 2.0
    # the extreme aspects can only be served by the fallback crop: 200 x 30 -> the full width and round(30 / (3/4)) = 40 rows
    tall = [r for (H, W), r in zip(hw, d.tolist()) if (H, W) == (200, 30)]
    assert any(r[:4] == [80.0, 0.0, 40.0, 30.0] for r in tall)
    wide = [r for (H, W), r in zip(hw, d.tolist()) if (H, W) == (30, 200)]
    assert any(r[:4] == [0.0, 80.0, 30.0, 40.0] for r in wide)
    # rates: prime blurs 10 % and solarises 20 %, the second view blurs always and never solarises
    n = len(hw)
    assert 0.3 < d[:, 4].mean() < 0.7 and 0.65 < (d[:, 5] >= 0).double().mean() < 0.95 and 0.08 < d[:, 13].mean() < 0.35
    assert (d[:, 14] > 0).double().mean() < 0.25 and 0.08 < d[:, 15].mean() < 0.35
    d2 = _views(which="second").draw_image_views(hw, torch.Generator().manual_seed(5))
    assert bool((d2[:, 14] >= 0.1).all()) and bool((d2[:, 15] == 0).all())
    assert torch.equal(d2[:, :14], d[:, :14])                  # the same uniforms decide the same stages
    # the clip chain draws nothing
    g = torch.Generator().manual_seed(5)
    dc = _views("clip").draw_image_views(hw[:3], g)
    assert torch.equal(torch.rand(2, generator=g), torch.rand(2, generator=torch.Generator().manual_seed(5)))
    assert dc[:, :4].tolist() == [[0, 0, 37, 53], [0, 0, 360, 640], [0, 0, 48, 64]] and bool((dc[:, 5] == -1).all()) and n > 0


def test_restated_resample_equals_pil_byte_for_byte(fx):
    frames = {}
    for name, (h, w, seed, noise, n) in ref.CLIP_CASES.items():
        f = ref.seeded_frame(h, w, seed, noise)
        assert int(f.astype(np.int64).sum()) == int(fx["sum_" + name]), name           # the seeded frame is the one PIL saw
        if "frame_" + name in fx.files:
            assert np.array_equal(f, fx["frame_" + name])
        frames[name] = f
        assert np.array_equal(ref.clip_u8(f, n), fx["clip_" + name]), name
    assert np.array_equal(fx["clip_32x32"], frames["32x32"])                            # the identity returns its input
    for key, (fname, box) in ref.BOX_CASES.items():
        assert np.array_equal(ref.box_u8(frames[fname], box, 32), fx["box_" + key]), key
    assert ref.clip_geometry(360, 640, 224) == (224, 398, 0, 87) and ref.clip_geometry(30, 200, 32) == (32, 213, 0, 90)
    assert ref.clip_geometry(5, 7, 32) == (32, 44, 0, 6) and ref.clip_geometry(200, 30, 32)[2] == 90        # (181 / 2 = 90.5 -> 90: half to even)
    assert max(len(k) for _, k in ref.coeffs(256, 32)) <= 33                           # the coefficient count at the downscale limit


def test_restated_photometric_stages_against_pil(fx):
    """From uint8 input: gray and solarise are PIL's; floor of brightness / contrast / saturation is PIL's wherever the value is not
    within 1e-3 of an integer (clipped values are exact and are compared); hue and blur stay within the distances DESIGN.md states."""
    for tag in ("noise", "smooth"):
        b = fx["base_" + tag].astype(np.float64)
        assert np.array_equal(ref.gray(b)[0][..., 0], fx["gray_" + tag]) and np.array_equal(ref.solarise(b)[0], fx["solar_" + tag])
        assert ref.contrast_mean(b)[0] == int(fx["contrast_deg_" + tag])
        for name, fn in (("bright", ref.brightness), ("contrast", ref.contrast), ("color", lambda x, a: ref.saturation(x, a)[0])):
            for i, f in enumerate(fx["factors"]):
                v = fn(b, float(f))
                fr = v - np.floor(v)
                ok = (np.minimum(fr, 1 - fr) > 1e-3) | (v == 0.0) | (v == 255.0)
                assert np.array_equal(np.floor(v)[ok], fx[f"{name}_{tag}"][i][ok]), (tag, name, f)
        for i, s in enumerate(fx["hues"]):
            d = np.abs(ref.hue(b, float(s)) - fx["hue_" + tag][i])
            assert d.mean() <= 1.6 and d.max() <= 14.0, (tag, s, d.mean(), d.max())
        for i, s in enumerate(fx["sigmas"]):
            d = np.abs(ref.blur(b, float(s)) - fx["blur_" + tag][i])
            assert d.mean() <= 1.1 and d.max() <= 3.0, (tag, s, d.mean(), d.max())
    x = np.random.RandomState(3).uniform(0, 255, (8, 8, 3))
    assert np.allclose(ref.hue(x, 0.0), x, atol=1e-9) and np.allclose(ref.hue(ref.hue(x, 0.3), -0.3), x, atol=1e-9)
    l, a = ref.blur_params(2.0)
    assert l == 1 and 0 < a < 1 and ref.blur_params(0.1)[0] == 0
    assert np.allclose(ref.blur(np.full((6, 6, 3), 77.0), 1.3), 77.0)


def test_chain_selection_from_the_config():
    from vipant_amd.config import compose
    from vipant_amd.image_views import ImageViews
    ov = ("+running=siamese worker=CVASP monitor=VASMonitor +model/image=vit_val +model/audio=vit_val +model/text=dummy "
          "+model/loss=ce_va +optimizer=standard +running/audio=default num_gpus=1")
    cfg = compose(ov.split())
    assert cfg.running.get("image_frames", None) is None                                # opt-in: no default
    p = ImageViews.from_config(cfg.running, True, "prime", device="cpu")
    s = ImageViews.from_config(cfg.running, True, "second", device="cpu")
    assert (p.chain, p.which, p.n_px, p.p_blur, p.p_solarise) == ("barlow", "prime", 224, 0.1, 0.2)
    assert (s.chain, s.which, s.p_blur, s.p_solarise) == ("barlow", "second", 1.0, 0.0)
    assert p.mean == (0.48145466, 0.4578275, 0.40821073) and p.std == (0.26862954, 0.26130258, 0.27577711)
    assert ImageViews.from_config(cfg.running, False, "prime", device="cpu").chain == "clip"           # evaluation is always clip
    tf = compose((ov + " running.clip_tf=True +running.image_frames=[48,64] model.image.resolution=32").split())
    assert list(tf.running.image_frames) == [48, 64]
    for which in ("prime", "second"):
        v = ImageViews.from_config(tf.running, True, which, device="cpu")
        assert v.chain == "clip" and v.n_px == 32
    bi = compose(ov.replace("+running=siamese", "+running=bimodal").split())
    assert ImageViews.from_config(bi.running, True, "prime", device="cpu").chain == "clip"             # the bimodal trainer
    assert ImageViews.from_config(cfg.running, True, "prime", device="cpu", siamese=False).chain == "clip"
    from vipant_amd._ffi import VipantError
    for bad in (dict(chain="simclr"), dict(which="third"), dict(n_px=225), dict(n_px=0), dict(std=(1.0, 0.0, 1.0))):
        with pytest.raises(VipantError):
            ImageViews(**{"n_px": 32, "device": "cpu", **bad})


def test_the_loader_yields_frames_only_under_the_key():
    from vipant_amd.config import compose
    from vipant_amd.monitor import SyntheticLoader
    ov = ("+running=siamese worker=CVASP monitor=VASMonitor +model/image=vit_val +model/audio=vit_val +model/text=dummy "
          "+model/loss=ce_va +optimizer=standard +running/audio=default num_gpus=1 running.batch_size=2 model.image.resolution=32 "
          "running.audio.max_len=64 running.audio.num_mel_bins=16")
    plain = list(SyntheticLoader(compose(ov.split()), 2, False))
    keyed = list(SyntheticLoader(compose((ov + " +running.image_frames=[48,64]").split()), 2, False))
    for a, b in zip(plain, keyed):
        assert a[1].dtype == torch.float32 and a[1].shape == (2, 3, 32, 32)
        assert b[1].dtype == torch.uint8 and b[1].shape == (2, 48, 64, 3) and b[1] is b[2]             # one frame, two views
        for k in (0, 3, 4):
            assert torch.equal(a[k], b[k])                                                             # the other slots keep their draws
    assert not torch.equal(keyed[0][1], keyed[1][1])
    again = list(SyntheticLoader(compose((ov + " +running.image_frames=[48,64]").split()), 2, False))
    assert torch.equal(again[1][1], keyed[1][1])
    bi = ov.replace("+running=siamese", "+running=bimodal") + " +running.image_frames=[48,64]"
    batch = next(iter(SyntheticLoader(compose(bi.split()), 1, False)))
    assert batch[0].dtype == torch.uint8 and batch[0].shape == (2, 48, 64, 3)


def test_refusals_that_need_no_device():
    from vipant_amd._ffi import VipantError
    v = _views("clip")
    with pytest.raises(VipantError, match="no CPU path"):
        v(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(VipantError, match="no CPU path"):
        v(np.zeros((1, 8, 8, 3), dtype=np.uint8))


def test_abi_symbols_and_workspace_query():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    lib = _ffi.lib()
    assert hasattr(lib, "vipant_image_view") and hasattr(lib, "vipant_image_view_workspace_bytes")
    assert _ffi.ABI_VERSION == lib.vipant_version() == 101                              # new exports, no bump

    def up(x):
        return (x + 255) // 256 * 256
    for b, n in ((1, 32), (3, 32), (512, 224)):
        want = up(up(up(up(up(b * 8) + b * 128) + b * 128) + b * 2 * n * 36 * 4) + b * n * n * 4)
        assert _ffi.query("vipant_image_view_workspace_bytes", b, n, 360, 640) == want
    assert _ffi.query("vipant_image_view_workspace_bytes", 1, 225, 8, 8) == 0 and _ffi.query("vipant_image_view_workspace_bytes", 0, 32, 8, 8) == 0
    # every refusal is made on the host, before the first launch: no device is needed to see it (and nothing can have been written)
    p = _ffi.ImageParams(32, (_ffi._f32 * 3)(0, 0, 0), (_ffi._f32 * 3)(1, 1, 1), 31)
    hw = (_ffi.C.c_int32 * 2)(257, 257)
    with pytest.raises(_ffi.VipantError, match="downscale limit"):
        _ffi.call("vipant_image_view", 256, 257 * 257 * 3, 257 * 3, 3, 257, 257, hw, None, p, 256, 1, 256, 1 << 30, None)
    hw = (_ffi.C.c_int32 * 2)(0, 5)
    with pytest.raises(_ffi.VipantError, match="outside"):
        _ffi.call("vipant_image_view", 256, 75, 15, 3, 5, 5, hw, None, p, 256, 1, 256, 1 << 30, None)
    hw = (_ffi.C.c_int32 * 2)(5, 5)
    row = (_ffi.C.c_double * 16)(2, 2, 4, 3, 0, -1, -1, -1, -1, 1, 1, 1, 0, 0, 0, 0)
    with pytest.raises(_ffi.VipantError, match="not an integer box inside"):
        _ffi.call("vipant_image_view", 256, 75, 15, 3, 5, 5, hw, row, p, 256, 1, 256, 1 << 30, None)
    with pytest.raises(_ffi.VipantError, match="workspace"):
        _ffi.call("vipant_image_view", 256, 75, 15, 3, 5, 5, hw, None, p, 256, 1, 256, 16, None)
    assert math.isfinite(1.0)


def test_registry_exclusions_still_hold():
    import cvap.module
    reg = cvap.module.LOSS_HEADS_REGISTRY
    for name in ("BCHingeLossHead", "ImagineAndClassifyLossHead", "LMLossHead"):
        assert name not in reg
