"""GPU image views: the image towers' input stage, decoded uint8 frames in, normalised fp32 [b, 3, n, n] out.

The reference does this per frame in loader processes, in PIL: the bimodal VA loader runs `make_clip_image_transform` --
Resize(bicubic) + CenterCrop + ToTensor + Normalize (cvap/data/image/transform.py:11-18, image_audio.py:117, 170-171) -- and the
siamese loader `BarlowImageTransform` (transform.py:146-200), or `AuthenticCLIPImageTransform` when `running.clip_tf` is set
(image_audio.py:232-237).  `ImageViews` does the same for a whole batch of device-resident frames in two launches (`clip`) or
three (`barlow`), `vipant_image_view` (csrc/image.hip): the resample is PIL's bicubic byte for byte, the photometric stages run on
fp32 code values without the re-quantisation PIL does between them.  The random draws are made on the host
(`draw_image_views`), a fixed number of uniforms per image whatever fires, as `KaldiFbank.draw_views` does.  Decoding stays with
the loader.

Chains:  `clip`    Resize(n) + CenterCrop(n) + Normalize (evaluation always; the bimodal and tagging trainers; both siamese views
                   under `running.clip_tf`)
         `barlow`  RandomResizedCrop(n, scale (0.08, 1), ratio (3/4, 4/3)), flip 0.5, ColorJitter(0.4, 0.4, 0.2, 0.1) with p = 0.8 in
                   a random order, gray 0.2, blur (sigma = U 1.9 + 0.1) with p = 0.1 for the prime view and 1.0 for the second,
                   solarise with p = 0.2 for the prime view and 0.0 for the second, Normalize
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import ops
from . import _ffi
from ._ffi import VipantError, call, query

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)          # transform.py:17
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
CHAINS = ("clip", "barlow")
VIEWS = ("prime", "second")
DRAW_COLUMNS = 16
# columns of a draw row (include/vipant_hip.h)
D_Y0, D_X0, D_H, D_W, D_FLIP, D_ORD0, D_FAC0, D_GRAY, D_SIGMA, D_SOLAR = 0, 1, 2, 3, 4, 5, 9, 13, 14, 15
UNIFORMS_PER_IMAGE = 54          # 10 tries x (area, ratio, top, left) + flip + jitter + 4 order keys + 4 factors + gray + blur + sigma + solarise
MAX_N = 224                      # the kernels' limit on n (per axis they also take at most 8 source pixels per resized pixel)
_ALL = _ffi.IMAGE_FLIP | _ffi.IMAGE_JITTER | _ffi.IMAGE_GRAY | _ffi.IMAGE_BLUR | _ffi.IMAGE_SOLARISE


def _py_round(v: float) -> int:
    return int(round(v))


class ImageViews:
    """uint8 frames [b, H, W, 3] on the device -> fp32 [b, 3, n_px, n_px]; see the module docstring for the chains."""

    def __init__(self, n_px: int = 224, chain: str = "clip", mean: Sequence[float] = CLIP_MEAN, std: Sequence[float] = CLIP_STD,
                 device="cuda:0", which: str = "prime"):
        if chain not in CHAINS:
            raise VipantError(f"image views: chain `{chain}' is not one of {', '.join(CHAINS)}")
        if which not in VIEWS:
            raise VipantError(f"image views: view `{which}' is not one of {', '.join(VIEWS)}")
        if not 1 <= int(n_px) <= MAX_N:
            raise VipantError(f"image views: n_px = {n_px} outside [1, {MAX_N}]")
        if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
            raise VipantError("image views: mean and std take three values each, std without zeros")
        self.n_px, self.chain, self.which = int(n_px), chain, which
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        self.device = torch.device(device)
        self.p_flip, self.p_jitter, self.p_gray = 0.5, 0.8, 0.2                 # transform.py:150-160
        self.p_blur, self.p_solarise = (0.1, 0.2) if which == "prime" else (1.0, 0.0)     # transform.py:161-162 / :177-178

    @classmethod
    def from_config(cls, rcfg, train: bool = True, which: str = "prime", device="cuda:0", siamese: bool = True):
        """`rcfg` = the `running` node.  `barlow` only for a training view of the siamese loader without `running.clip_tf`
        (image_audio.py:232-237); `clip` for everything else, evaluation included."""
        res = rcfg.get("resolution", 224)
        if isinstance(res, (list, tuple)):
            res = 224
        barlow = bool(train) and bool(siamese) and bool(rcfg.get("multi_view", False)) and not bool(rcfg.get("clip_tf", False))
        return cls(int(res), "barlow" if barlow else "clip", device=device, which=which)

    # ---- draws -----------------------------------------------------------------------------------------------------------------
    def draw_image_views(self, hw, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """hw [b, 2] (h, w) per frame -> host fp64 [b, 16]: the box (top, left, height, width) and the flip flag, the order of the
        four jitter operations (0 brightness, 1 contrast, 2 saturation, 3 hue; -1 in the first slot when jitter is off), their four
        factors, the gray flag, sigma (0 = off) and the solarise flag.  UNIFORMS_PER_IMAGE uniforms per image whatever fires.  The
        `clip` chain draws nothing: its rows hold the whole frame and fire nothing (`__call__` does not need them)."""
        hw = torch.as_tensor(hw).reshape(-1, 2).tolist()
        b = len(hw)
        draws = torch.zeros(b, DRAW_COLUMNS, dtype=torch.float64)
        draws[:, D_ORD0:D_ORD0 + 4] = -1.0
        draws[:, D_FAC0:D_FAC0 + 3] = 1.0
        if self.chain == "clip":
            for i, (H, W) in enumerate(hw):
                draws[i, D_H], draws[i, D_W] = float(H), float(W)
            return draws
        u = torch.rand(b, UNIFORMS_PER_IMAGE, generator=generator, dtype=torch.float64).tolist()
        lo, hi = math.log(3.0 / 4.0), math.log(4.0 / 3.0)
        for i, (H, W) in enumerate(hw):
            H, W, ui = int(H), int(W), u[i]
            box = None
            for t in range(10):                                                  # RandomResizedCrop.get_params
                area = H * W * (0.08 + ui[4 * t] * (1.0 - 0.08))
                ratio = math.exp(lo + ui[4 * t + 1] * (hi - lo))
                w, h = _py_round(math.sqrt(area * ratio)), _py_round(math.sqrt(area / ratio))
                if box is None and 0 < w <= W and 0 < h <= H:
                    box = (min(int(ui[4 * t + 2] * (H - h + 1)), H - h), min(int(ui[4 * t + 3] * (W - w + 1)), W - w), h, w)
            if box is None:                                                      # the central crop clamped to the ratio bounds
                in_ratio = float(W) / float(H)
                if in_ratio < 3.0 / 4.0:
                    w, h = W, _py_round(W / (3.0 / 4.0))
                elif in_ratio > 4.0 / 3.0:
                    h, w = H, _py_round(H * (4.0 / 3.0))
                else:
                    w, h = W, H
                h, w = min(h, H), min(w, W)
                box = ((H - h) // 2, (W - w) // 2, h, w)
            row = [float(v) for v in box] + [float(ui[40] < self.p_flip)]
            if ui[41] < self.p_jitter:
                order = sorted(range(4), key=lambda k: ui[42 + k])
                row += [float(k) for k in order]
                row += [0.6 + 0.8 * ui[46], 0.6 + 0.8 * ui[47], 0.8 + 0.4 * ui[48], -0.1 + 0.2 * ui[49]]
            else:
                row += [-1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 0.0]
            row += [float(ui[50] < self.p_gray), (ui[52] * 1.9 + 0.1) if ui[51] < self.p_blur else 0.0,
                    float(ui[53] < self.p_solarise)]
            draws[i] = torch.tensor(row, dtype=torch.float64)
        return draws

    # ---- the launch ------------------------------------------------------------------------------------------------------------
    def __call__(self, frames: torch.Tensor, hw=None, draws: Optional[torch.Tensor] = None, chain_flags: Optional[int] = None,
                 out: Optional[torch.Tensor] = None):
        """frames uint8 [b, Hmax, Wmax, 3] on the device; hw [b, 2] the (h, w) of each frame inside it (default: all of it);
        draws host fp64 [b, 16] (`draw_image_views`), None = the `clip` chain.  -> fp32 [b, 3, n_px, n_px] (`out` when given: a
        contiguous fp32 device tensor of that shape).  `chain_flags` (_ffi.IMAGE_*) narrows the stages of the `barlow` chain."""
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda:
            raise VipantError("image views: frames must be a device tensor (there is no CPU path)")
        if frames.dtype != torch.uint8:
            raise VipantError(f"image views: frames must be uint8, got {frames.dtype}")
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise VipantError(f"image views: frames must be [b, H, W, 3], got {tuple(frames.shape)}")
        if frames.stride(3) != 1:
            frames = frames.contiguous()
        b, max_h, max_w = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
        if hw is None:
            hw = torch.tensor([[max_h, max_w]] * b, dtype=torch.int32)
        hw = torch.as_tensor(hw).to(device="cpu", dtype=torch.int32).contiguous()
        if hw.shape != (b, 2):
            raise VipantError(f"image views: hw must have shape [{b}, 2], got {tuple(hw.shape)}")
        if draws is None and self.chain != "clip":
            raise VipantError("image views: the `barlow' chain needs draws (draw_image_views)")
        if draws is not None:
            draws = torch.as_tensor(draws).to(device="cpu", dtype=torch.float64).contiguous()
            if draws.shape != (b, DRAW_COLUMNS):
                raise VipantError(f"image views: draws must have shape [{b}, {DRAW_COLUMNS}], got {tuple(draws.shape)}")
        flags = int(chain_flags) if chain_flags is not None else (_ALL if self.chain == "barlow" else 0)
        dev = frames.device
        params = _ffi.ImageParams(self.n_px, (_ffi._f32 * 3)(*self.mean), (_ffi._f32 * 3)(*self.std), flags)
        if out is None:
            out = torch.empty((b, 3, self.n_px, self.n_px), dtype=torch.float32, device=dev)
        elif (not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != (b, 3, self.n_px, self.n_px)
              or not out.is_contiguous()):
            raise VipantError(f"image views: out must be a contiguous fp32 device tensor [{b}, 3, {self.n_px}, {self.n_px}]")
        ws = ops.scratch("image_view", query("vipant_image_view_workspace_bytes", b, self.n_px, max_h, max_w), dev)
        call("vipant_image_view", frames.data_ptr(), frames.stride(0), frames.stride(1), frames.stride(2), max_h, max_w,
             hw.data_ptr(), draws.data_ptr() if draws is not None else None, params, out.data_ptr(), b, ws.data_ptr(), ws.numel(),
             ops._stream())
        self._host = (hw, draws)         # the launch copies the host arrays on the stream: they stay alive until the next call
        return out
