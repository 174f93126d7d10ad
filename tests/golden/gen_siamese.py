"""Inputs and configurations of the VACELossHead fixtures by name, shared by the generator (make_golden_siamese.py, which runs the
reference) and the tests: nothing but the reference's outputs is stored."""
from types import SimpleNamespace as NS

import torch

import gen

E = 512
KEYS = ("vp", "ap", "va", "vv", "aa")
SCALES = dict(vp=2.0, ap=2.3, va=2.6593, vv=3.1, aa=2.5)
MARGIN = 5e-5          # relative: the kernel's bound on a per-pair loss, which a `stats` value must clear to its rounding boundary
CASES = {      # tag: (B, config overrides)
    "vace_default": (48, {}),
    "vace_all": (130, dict(ap=True, aa=True, vp_w=1., ap_w=.5, va_w=2., vv_w=.25, aa_w=1.5, scale_max=18.0)),
}


def loss_cfg(**over):
    cfg = dict(name="VACELossHead", layers=[], scaling=True, scale_max=None, vp=True, vp_w=1., ap=False, ap_w=1., va=True, va_w=1.,
               vv=True, vv_w=1., aa=False, aa_w=1.)
    cfg.update(over)
    return NS(**cfg)


def vace_inputs(tag, B, noise=3.0):
    """(prime, image view 1, audio view 1, image view 2, audio view 2): un-normalised, a shared clip signal under independent noise."""
    base = gen.det_randn(f"{tag}/base", (B, E))
    return [base + noise * gen.det_randn(f"{tag}/{n}", (B, E)) for n in ("prime", "v1", "a1", "v2", "a2")]


def set_scales(head):
    with torch.no_grad():
        for k in KEYS:
            sub = getattr(head, f"loss_head_{k}")
            if sub is not None:
                sub.logit_scale.fill_(SCALES[k])


def e2e_views(tag, b):
    """Two image views of one frame per clip under independent noise, [b, 3, 224, 224] each."""
    frames = gen.det_randn(f"{tag}/frames", (b, 3, 224, 224))
    return (frames + 0.5 * gen.det_randn(f"{tag}/v1", (b, 3, 224, 224)), frames + 0.5 * gen.det_randn(f"{tag}/v2", (b, 3, 224, 224)))
