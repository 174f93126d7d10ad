"""CVASP worker: siamese multi-view vision-audio pre-training (`worker=CVASP`, cvap/model/siamese_va.py:29-153).

Per step: pre-computed "prime" image features, two image views through the (trainable) image tower, one audio view through the
audio tower, and VACELossHead over them.  Two points of fidelity with the reference's forward:
  * `audios_v2` is never encoded: the loss head receives the second IMAGE view's features in that slot (siamese_va.py:62-65);
  * the reference calls the image tower once per view; here both views go through it as ONE batch of 2 b rows (one stack node,
    twice the rows per launch, one gradient bucket per block) and are split after the read-out.  Every operator of the tower
    treats samples independently, so the features are those of two passes, bit for bit (tests/test_siamese_gpu.py).
"""
from __future__ import annotations

import torch

from .. import ops
from ..module import build_audio_head, build_image_head, build_loss_head, build_text_head
from .cvalp import CVALP
from .helper import load_checkpoint, load_clip


class CVASP(CVALP):
    def forward(self, images, images_v1, audios_v1, text_v1=None, images_v2=None, audios_v2=None, *args, **kwargs):
        kwargs = {"normalized": self.loss_head.normalized, "names": kwargs.get("names", None)}
        image_features = image_features_v1 = image_features_v2 = audio_features_v1 = None
        if images is not None:                         # pre-computed un-normalised features
            dummy_image = list(images.shape[1:]) == [1, 1, 1]
            if self.loss_head.normalized and not dummy_image:
                images = ops.l2_normalize(images)
            image_features = images
        if self.image_head is not None:
            image_features_v1, image_features_v2 = self.encode_views(images_v1, images_v2, **kwargs)
        if audios_v1 is not None and self.audio_head is not None:
            audio_features_v1 = self.audio_head(audios_v1, **kwargs)
        if text_v1 is not None and self.text_head is not None:
            self.text_head(text_v1, **kwargs)          # (the reference encodes the text and drops the features)
        return self.loss_head(image_features, image_features_v1, audio_features_v1, images_v2=image_features_v2,
                              audios_v2=image_features_v2, **kwargs)

    def encode_views(self, images_v1, images_v2, **kwargs):
        """Both image views through the image tower as one batch; (features of view 1, of view 2), None for an absent view."""
        views = [v for v in (images_v1, images_v2) if v is not None]
        if not views:
            return None, None
        with torch.set_grad_enabled(torch.is_grad_enabled() and not self._frozen(self.image_head)):
            feats = self.image_head(torch.cat(views) if len(views) > 1 else views[0], **kwargs)
        parts = list(feats.split([v.shape[0] for v in views]))
        return (parts.pop(0) if images_v1 is not None else None), (parts.pop(0) if images_v2 is not None else None)

    def _build_siamese_backbone(self, **kwargs):
        """siamese_va.py:68-153: the image head is the reference of the shared modules and is never destroyed; parameters it shares
        with the audio / text heads stay tunable when the image tower is frozen (CVALP._tunable)."""
        cfg = self.cfg
        local_cfg, _, audio_head_sd, _, loss_head_sd = load_checkpoint(cfg, self.echo)
        from_scratch, image_head_sd, text_head_sd, _ = load_clip(None, cfg, self.echo)
        self.image_head = build_image_head(cfg.model.image)
        if not from_scratch and not cfg.model.image.from_scratch:
            n_o, _ = self.image_head.copy_state_dict(image_head_sd)
            self._init_msg("image", "image_head", n_o)
        scfg = cfg.running.siamese
        amodules = set(scfg.amodules)
        skw = {"shared_modules": amodules, "reference": self.image_head, "keep_hp": scfg.keep_hp}
        self.audio_head = build_audio_head(cfg.model.audio, **skw)
        if not cfg.model.audio.from_scratch:
            if local_cfg is not None:
                n_o, _ = self.audio_head.from_pretrained(audio_head_sd, local_cfg)
                self._init_msg("audio", "audio_head", n_o)
            elif not from_scratch:
                n_o, _ = self.audio_head.copy_state_dict(image_head_sd)
                self._init_msg("audio", "image_head", n_o)
            else:
                self.echo("Have to learn from scratch.")
        ref_modules = self.audio_head.replace_modules(**skw)
        self.echo(f"A: audio_head.modules referring to image_head.modules: {ref_modules}.")
        lmodules = set(scfg.lmodules)
        skw.update({"shared_modules": lmodules})
        self.text_head = build_text_head(cfg.model.text, **skw)
        if not from_scratch and not cfg.model.text.from_scratch:
            src = text_head_sd if cfg.model.text.from_text else image_head_sd
            n_o, _ = self.text_head.copy_state_dict(src)
            self._init_msg("text", "text_head" if cfg.model.text.from_text else "image_head", n_o)
        ref_modules = self.text_head.replace_modules(**skw)
        self.echo(f"T:  text_head.modules referring to image_head.modules: {ref_modules}.")
        if len(self.text_head.state_dict()) == 0:
            self.text_head = None
            self.echo("Destory text encoder.")
        self.loss_head = build_loss_head(cfg.model.loss, **kwargs)
        return self._tunable(lmodules, amodules)
