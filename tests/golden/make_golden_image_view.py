"""Writes tests/golden/image_view.npz: what PIL computes for the image-view cases (PIL and numpy only; run by hand).

    python tests/golden/make_golden_image_view.py

Frames come from tests/image_view_ref.py (seeded, integer arithmetic); the small ones are stored, the large ones only as a byte sum.
Every stage result is PIL's uint8 output from that stage's own uint8 input."""
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageFilter, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import image_view_ref as ref  # noqa: E402

FACTORS = (0.613, 0.77, 0.83, 1.17, 1.23, 1.387)
HUES = (-0.1, -0.037, 0.021, 0.1)
SIGMAS = (0.1, 0.7, 1.3, 2.0)


def pil_clip(frame, n):
    h, w = frame.shape[:2]
    oh, ow, top, left = ref.clip_geometry(h, w, n)
    im = Image.fromarray(frame).resize((ow, oh), Image.BICUBIC)
    return np.asarray(im.crop((left, top, left + n, top + n)))


def pil_box(frame, box, n):
    y0, x0, h, w = box
    return np.asarray(Image.fromarray(frame).crop((x0, y0, x0 + w, y0 + h)).resize((n, n), Image.BICUBIC))


def pil_hue(im, shift):
    h, s, v = im.convert("HSV").split()
    nh = (np.asarray(h).astype(np.int64) + int(shift * 255)) % 256
    return np.asarray(Image.merge("HSV", (Image.fromarray(nh.astype(np.uint8), "L"), s, v)).convert("RGB"))


def main():
    out = {}
    frames = {}
    for name, (h, w, seed, noise, n) in ref.CLIP_CASES.items():
        f = ref.seeded_frame(h, w, seed, noise)
        frames[name] = f
        if f.size <= 3 * 64 * 64:
            out["frame_" + name] = f
        out["sum_" + name] = np.int64(f.astype(np.int64).sum())
        out["clip_" + name] = pil_clip(f, n)
    for key, (fname, box) in ref.BOX_CASES.items():
        out["box_" + key] = pil_box(frames[fname], box, 32)
    # photometric stages from uint8 input: a noise frame (the 32 x 32 box at (8, 16) of a 48 x 64 one) and a smooth one
    noise = ref.seeded_frame(48, 64, 31, 255)
    out["frame_48x64"] = noise
    base = {"noise": np.ascontiguousarray(noise[8:40, 16:48]), "smooth": ref.seeded_frame(32, 32, 32, 0)}
    out["blocks32"] = ref.block_frame(32, 33)
    for tag, arr in base.items():
        im = Image.fromarray(arr)
        out[f"base_{tag}"] = arr
        out[f"gray_{tag}"] = np.asarray(im.convert("L"))
        out[f"solar_{tag}"] = np.asarray(ImageOps.solarize(im, 128))
        out[f"bright_{tag}"] = np.stack([np.asarray(ImageEnhance.Brightness(im).enhance(f)) for f in FACTORS])
        out[f"contrast_{tag}"] = np.stack([np.asarray(ImageEnhance.Contrast(im).enhance(f)) for f in FACTORS])
        out[f"contrast_deg_{tag}"] = np.asarray(ImageEnhance.Contrast(im).enhance(0.0))[0, 0, 0]
        out[f"color_{tag}"] = np.stack([np.asarray(ImageEnhance.Color(im).enhance(f)) for f in FACTORS])
        out[f"hue_{tag}"] = np.stack([pil_hue(im, s) for s in HUES])
        out[f"blur_{tag}"] = np.stack([np.asarray(im.filter(ImageFilter.GaussianBlur(s))) for s in SIGMAS])
    out["factors"], out["hues"], out["sigmas"] = np.asarray(FACTORS), np.asarray(HUES), np.asarray(SIGMAS)
    path = os.path.join(HERE, "image_view.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
