"""Host restatement of the image-view semantics (numpy, fp64): what csrc/image.hip has to compute, written from the rules and from
PIL's own arithmetic -- never from the kernels.  The resample part is integer exact (PIL's fixed-point bicubic, byte for byte, which
tests/test_image_view_cpu.py checks against tests/golden/image_view.npz); the photometric stages are the same formulas in fp64,
without any quantisation in between, together with a mask of the pixels where an fp32 evaluation may legitimately take the other side
of a discontinuity (a gray rounding tie, the solarise threshold)."""
import math

import numpy as np

TIE = 1e-2          # a pixel within this of a gray rounding tie or of the solarise threshold is flagged
D_Y0, D_X0, D_H, D_W, D_FLIP, D_ORD0, D_FAC0, D_GRAY, D_SIGMA, D_SOLAR = 0, 1, 2, 3, 4, 5, 9, 13, 14, 15
FLIP, JITTER, GRAY, BLUR, SOLARISE = 1, 2, 4, 8, 16
ALL = 31


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def py_round_half(d: int) -> int:
    return int(round(d / 2.0))


def clip_geometry(H: int, W: int, n: int):
    """Resize(n) + CenterCrop(n) -> (resized h, resized w, crop top, crop left)."""
    if W <= H:
        ow, oh = n, int(n * H / W)
    else:
        oh, ow = n, int(n * W / H)
    return oh, ow, py_round_half(oh - n), py_round_half(ow - n)


def _bicubic(x: float) -> float:
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size: int, out_size: int, first: int = 0, count=None):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for output indices [first, first + count) -> [(xmin, int coefficients)]."""
    count = out_size - first if count is None else count
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    out = []
    for i in range(first, first + count):
        center = (i + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5))
        w = [_bicubic((x - center + 0.5) * ss) for x in range(xmin, xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]
        out.append((xmin, np.asarray(k, dtype=np.int64)))
    return out


def _pass(img: np.ndarray, table) -> np.ndarray:
    """one pass along axis 1 of uint8 [rows, in, 3] -> uint8 [rows, len(table), 3]"""
    out = np.empty((img.shape[0], len(table), img.shape[2]), dtype=np.uint8)
    src = img.astype(np.int64)
    for j, (xmin, k) in enumerate(table):
        acc = (1 << 21) + np.tensordot(src[:, xmin:xmin + len(k), :], k, axes=([1], [0]))
        out[:, j, :] = np.clip(acc >> 22, 0, 255)
    return out


def resample_u8(img: np.ndarray, oh: int, ow: int, top: int = 0, left: int = 0, n_h=None, n_w=None) -> np.ndarray:
    """Image.resize((ow, oh), BICUBIC) of uint8 [h, w, 3], restricted to the output window (top, left, n_h, n_w)."""
    n_h = oh - top if n_h is None else n_h
    n_w = ow - left if n_w is None else n_w
    hor = _pass(img, coeffs(img.shape[1], ow, left, n_w))                       # horizontal first, uint8 in between
    return _pass(hor.transpose(1, 0, 2), coeffs(img.shape[0], oh, top, n_h)).transpose(1, 0, 2)


def clip_u8(frame: np.ndarray, n: int) -> np.ndarray:
    oh, ow, top, left = clip_geometry(frame.shape[0], frame.shape[1], n)
    return resample_u8(frame, oh, ow, top, left, n, n)


def box_u8(frame: np.ndarray, box, n: int, flip: bool = False) -> np.ndarray:
    y0, x0, h, w = (int(v) for v in box)
    out = resample_u8(frame[y0:y0 + h, x0:x0 + w], n, n)
    return out[:, ::-1] if flip else out


def normalise32(codes: np.ndarray, mean, std) -> np.ndarray:
    """ToTensor + Normalize as three rounded fp32 operations; codes [n, n, 3] -> [3, n, n]"""
    v = codes.astype(np.float32) / np.float32(255.0)
    v = (v - np.asarray(mean, dtype=np.float32)) / np.asarray(std, dtype=np.float32)
    return np.ascontiguousarray(v.transpose(2, 0, 1))


# ---- photometric stages, fp64 on code values [n, n, 3] ----------------------------------------------------------------------------
def luma(x: np.ndarray):
    """-> (L, near): PIL's convert("L") rule and the pixels within TIE of a rounding tie"""
    t = (19595.0 * x[..., 0] + 38470.0 * x[..., 1] + 7471.0 * x[..., 2]) / 65536.0 + 0.5
    L = np.floor(t)
    frac = t - L
    return L, np.minimum(frac, 1.0 - frac) < TIE


def _blend(deg, alpha, x):
    return np.clip(deg + alpha * (x - deg), 0.0, 255.0)


def brightness(x, alpha):
    return _blend(0.0, alpha, x)


def contrast_mean(x):
    """-> (degenerate value, the mean before rounding)"""
    m = float(luma(x)[0].sum()) / float(x.shape[0] * x.shape[1])
    return math.floor(m + 0.5), m


def contrast(x, alpha):
    return _blend(float(contrast_mean(x)[0]), alpha, x)


def saturation(x, alpha):
    L, near = luma(x)
    return _blend(L[..., None], alpha, x), near


def hue(x, shift):
    """Python's colorsys, vectorised: rgb -> hsv, h = frac(h + shift), -> rgb"""
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    rng = maxc - minc
    flat = rng == 0.0
    safe = np.where(flat, 1.0, rng)
    s = np.where(flat, 0.0, rng / np.where(maxc == 0.0, 1.0, maxc))
    rc, gc, bc = (maxc - r) / safe, (maxc - g) / safe, (maxc - b) / safe
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
    h = (h / 6.0) % 1.0
    h = (h + shift) % 1.0
    h6 = h * 6.0
    i = np.floor(h6).astype(np.int64)
    f = h6 - i
    v = maxc
    p, q, t = v * (1.0 - s), v * (1.0 - s * f), v * (1.0 - s * (1.0 - f))
    i = i % 6
    rr = np.choose(i, [v, q, p, p, t, v])
    gg = np.choose(i, [t, v, v, q, p, p])
    bb = np.choose(i, [p, p, t, v, v, q])
    out = np.stack([rr, gg, bb], axis=-1)
    return np.where(flat[..., None], x, out)


def gray(x):
    L, near = luma(x)
    return np.repeat(L[..., None], 3, axis=-1), near


def blur_params(sigma: float):
    s2 = sigma * sigma / 3.0
    L = math.sqrt(12.0 * s2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2.0 * l + 1.0) * (l * (l + 1.0) - 3.0 * s2) / (6.0 * (s2 - (l + 1.0) * (l + 1.0)))
    return int(l), a


def _box_pass(x, l, a, axis):
    n = x.shape[axis]
    idx = np.arange(n)
    acc = np.zeros_like(x)
    for d in range(-l, l + 1):
        acc = acc + np.take(x, np.clip(idx + d, 0, n - 1), axis=axis)
    outer = np.take(x, np.clip(idx - l - 1, 0, n - 1), axis=axis) + np.take(x, np.clip(idx + l + 1, 0, n - 1), axis=axis)
    return (acc + a * outer) / (2.0 * (l + a) + 1.0)


def blur(x, sigma):
    """PIL's GaussianBlur(sigma): three extended box passes along the rows, then three along the columns, clamp to the edge"""
    l, a = blur_params(sigma)
    for axis in (1, 1, 1, 0, 0, 0):
        x = _box_pass(x, l, a, axis)
    return x


def solarise(x):
    return np.where(x >= 128.0, 255.0 - x, x), (np.abs(x - 128.0) < TIE).any(axis=-1)


def _dilate(mask, r):
    out = mask.copy()
    n0, n1 = mask.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, xs = slice(max(dy, 0), n0 + min(dy, 0)), slice(max(dx, 0), n1 + min(dx, 0))
            yd, xd = slice(max(-dy, 0), n0 + min(-dy, 0)), slice(max(-dx, 0), n1 + min(-dx, 0))
            out[yd, xd] |= mask[ys, xs]
    return out


def photometric(codes: np.ndarray, row, flags: int = ALL):
    """The photometric part of a draw row on code values [n, n, 3] (after crop, resample and flip) -> (fp64 code values, mask of
    flagged pixels, [the contrast means before rounding]).  A jitter operation with a neutral factor is skipped, as in the kernel.
    A flagged pixel spreads through the blur to everything its value reaches."""
    x = codes.astype(np.float64)
    near = np.zeros(x.shape[:2], dtype=bool)
    means = []
    if (flags & JITTER) and row[D_ORD0] >= 0:
        for q in range(4):
            op = int(row[D_ORD0 + q])
            fac = float(np.float32(row[D_FAC0 + op]))          # the plan carries the factors as fp32
            if fac == (0.0 if op == 3 else 1.0):
                continue
            if op == 0:
                x = brightness(x, fac)
            elif op == 1:
                means.append(contrast_mean(x)[1])
                x = contrast(x, fac)
            elif op == 2:
                x, m = saturation(x, fac)
                near |= m
            else:
                x = hue(x, fac)
    if (flags & GRAY) and row[D_GRAY] != 0:
        x, m = gray(x)
        near |= m
    if (flags & BLUR) and row[D_SIGMA] > 0:
        x = blur(x, float(row[D_SIGMA]))
        near = _dilate(near, 3 * (blur_params(float(row[D_SIGMA]))[0] + 1))
    if (flags & SOLARISE) and row[D_SOLAR] != 0:
        x, m = solarise(x)
        near |= m
    return x, near, means


def view(frame: np.ndarray, row, n: int, flags: int = ALL):
    """A whole draw row: crop, resample, flip, photometric -> (fp64 code values [n, n, 3], flagged pixels, contrast means)"""
    codes = box_u8(frame, row[D_Y0:D_Y0 + 4], n, bool((flags & FLIP) and row[D_FLIP] != 0))
    return photometric(codes, row, flags)


def make_row(box, flip=0, order=None, factors=(1.0, 1.0, 1.0, 0.0), gray_on=0, sigma=0.0, solar=0):
    row = np.zeros(16, dtype=np.float64)
    row[D_Y0:D_Y0 + 4] = box
    row[D_FLIP] = flip
    row[D_ORD0:D_ORD0 + 4] = order if order is not None else (-1, -1, -1, -1)
    row[D_FAC0:D_FAC0 + 4] = factors
    row[D_GRAY], row[D_SIGMA], row[D_SOLAR] = gray_on, sigma, solar
    return row


# ---- seeded frames (integer arithmetic only: the same bytes on every machine) -----------------------------------------------------
def seeded_frame(h: int, w: int, seed: int, noise: int = 96) -> np.ndarray:
    """uint8 [h, w, 3]: three sawtooth ramps plus uniform noise of the given amplitude (0 = smooth, 255 = noise only)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([(yy * (3 + c) + xx * (5 - c) + 70 * c) % 256 for c in range(3)], axis=-1).astype(np.int64)
    ramp = np.where(ramp > 127, 255 - ramp, ramp) * 2                   # a triangle wave: no jumps
    if noise >= 255:
        return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    nz = rs.randint(0, noise + 1, (h, w, 3)) if noise > 0 else 0
    return np.clip((ramp * (255 - noise)) // 255 + nz, 0, 255).astype(np.uint8)


def block_frame(n: int, seed: int, cell: int = 8) -> np.ndarray:
    """uint8 [n, n, 3] of constant cells: few distinct colours, so that few pixels can sit near a rounding tie"""
    rs = np.random.RandomState(seed)
    k = (n + cell - 1) // cell
    cols = rs.randint(0, 256, (k, k, 3)).astype(np.uint8)
    return np.repeat(np.repeat(cols, cell, axis=0), cell, axis=1)[:n, :n]


# the resample cases of the fixture: name -> (h, w, seed, noise, n)
CLIP_CASES = {
    "1x1": (1, 1, 11, 255, 32), "5x7": (5, 7, 12, 255, 32), "7x5": (7, 5, 13, 255, 32), "37x53": (37, 53, 14, 255, 32),
    "53x37": (53, 37, 15, 96, 32), "32x32": (32, 32, 16, 255, 32), "30x200": (30, 200, 17, 96, 32), "200x30": (200, 30, 18, 255, 32),
    "256x256": (256, 256, 19, 96, 32),          # exactly at the downscale limit of 8 per axis
    "360x640": (360, 640, 20, 64, 224),         # the one full-size case
}
# crop boxes (top, left, height, width) resampled to 32 x 32: odd sizes, upscales, a box touching every border, a 1-pixel box, the
# identity, a box at the downscale limit
BOX_CASES = {
    "a": ("37x53", (3, 5, 29, 41)), "b": ("37x53", (0, 0, 37, 53)), "c": ("37x53", (30, 46, 7, 7)), "d": ("5x7", (1, 2, 3, 4)),
    "e": ("37x53", (36, 52, 1, 1)), "f": ("53x37", (10, 2, 32, 32)), "g": ("256x256", (0, 0, 256, 256)), "h": ("30x200", (2, 100, 28, 37)),
}
