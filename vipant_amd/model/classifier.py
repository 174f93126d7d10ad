"""Supervised audio classification workers (`worker=ESClassifier`, `worker=ASClassifier`) with the reference's build / forward /
state-dict contract (cvap/model/esc50_clf.py:29-128, cvap/model/audioset_clf.py:28-174).

ESClassifier: audio tower + ClassificationHead (ESC-50 / UrbanSound8K fine-tuning and linear probing, zero-shot through the text
tower).  ASClassifier: audio tower (+ optional image tower) + BCELossHead (AudioSet tagging).  Initialisation order of the audio
tower, as in the reference: a VA / AT checkpoint (`from_pretrained`: the positional grid is re-sliced for another clip length),
else CLIP's image tower, else from scratch.  `load_meme` (a torch.hub download) has no counterpart.
"""
from __future__ import annotations

import contextlib
import re

import torch
import torch.distributed as dist
from torch import nn

from .. import ops
from ..module import build_audio_head, build_image_head, build_loss_head, build_text_head
from .helper import load_checkpoint, load_clip


def _frozen(head) -> bool:
    return not any(p.requires_grad for p in head.parameters())


class _Classifier(nn.Module):
    def __init__(self, cfg, echo):
        super().__init__()
        self.cfg = cfg
        self.echo = echo

    def _device(self):
        if not torch.cuda.is_available():       # construction and state-dict surgery can be inspected on a CPU host
            return torch.device("cpu")
        return torch.device("cuda", torch.cuda.current_device())

    def _audio_features(self, audios, **kwargs):
        """A frozen tower (linear probe) has no place in the autograd tape: it runs under no_grad and takes the inference path."""
        if self.training and _frozen(self.audio_head):
            with torch.no_grad():
                return self.audio_head(audios, **kwargs)
        return self.audio_head(audios, **kwargs)

    def encode_audio(self, audios, *args, **kwargs):
        kwargs.pop("device_ids", None)
        return self.audio_head(audios, **kwargs)

    def encode_text(self, text, *args, **kwargs):
        kwargs.pop("device_ids", None)
        return self.text_head(text, **kwargs)

    def collect_audio_state_dict(self):
        return (self.audio_head.state_dict(), self.loss_head.state_dict())

    def _init_msg(self, what, src, n_o):
        msg = f" except {n_o}" if len(n_o) > 0 else ""
        self.echo(f"Initialize {what} encoder from `{src}`{msg}.")

    def _init_audio(self, local_cfg, audio_head_sd, image_head_sd, from_scratch):
        if audio_head_sd is not None and local_cfg is not None:
            n_o, _ = self.audio_head.from_pretrained(audio_head_sd, local_cfg)
            self._init_msg("audio", "audio_head", n_o)
        elif not from_scratch and image_head_sd is not None:
            n_o, _ = self.audio_head.copy_state_dict(image_head_sd)
            self._init_msg("audio", "image_head", n_o)
        else:
            self.echo("Have to learn from scratch.")

    def _tunable_audio(self, tunable_params):
        if not self.cfg.model.audio.freeze:
            excl_modules = set(self.cfg.running.excl_modules.amodules)
            pattern = "|".join([rf"^{m}\." for m in excl_modules])
            tunable_params.update({f"audio_head.{k}": v for k, v in self.audio_head.named_parameters()
                                   if pattern == "" or not re.match(pattern, k)})      # excluded sub-modules stay frozen
            self.echo(f"Tune audio encoder (excl. {excl_modules}).")
        else:
            self.echo("Freeze audio encoder.")
        return tunable_params


class ESClassifier(_Classifier):
    """cvap/model/esc50_clf.py:29-128."""

    image_head = None

    def forward(self, audios, labels, *args, **kwargs):
        kwargs = {"normalized": self.loss_head.normalized, "names": kwargs.get("names", None)}
        audio_features = self._audio_features(audios, **kwargs)
        return self.loss_head(audio_features, labels, **kwargs)

    def report(self, gold_file=None, **kwargs):
        if not dist.is_initialized() or dist.get_rank() == 0:
            return self.loss_head.report(gold_file=gold_file, **kwargs)
        return ""

    def build(self, **kwargs):
        tunable_params = dict()
        cfg = self.cfg
        loss_kwargs = {k: v for k, v in kwargs.items() if k in ("output_dim",)}
        local_cfg, _, audio_head_sd, _, loss_head_sd = load_checkpoint(cfg, self.echo)
        from_scratch, image_head_sd, text_head_sd, _ = load_clip(None, cfg, self.echo)
        self.audio_head = build_audio_head(cfg.model.audio)
        if cfg.eval:
            self._init_audio(local_cfg, audio_head_sd, image_head_sd, from_scratch)
            self.text_head = build_text_head(cfg.model.text)
            if text_head_sd is not None:
                n_o, _ = self.text_head.copy_state_dict(text_head_sd)
                self._init_msg("text", "text_head", n_o)
            self.loss_head = build_loss_head(cfg.model.loss, **loss_kwargs)
            if loss_head_sd is not None:
                self.loss_head.copy_state_dict(loss_head_sd)
        else:
            if not cfg.model.audio.from_scratch:
                self._init_audio(local_cfg, audio_head_sd, image_head_sd, from_scratch)
            self.loss_head = build_loss_head(cfg.model.loss, **loss_kwargs)
            tunable_params = {f"loss_head.{k}": v for k, v in self.loss_head.named_parameters()}
            self._tunable_audio(tunable_params)
        self.to(self._device())
        return tunable_params


class ASClassifier(_Classifier):
    """cvap/model/audioset_clf.py:28-174."""

    def forward(self, images, audios, labels, *args, **kwargs):
        kwargs = {"normalized": self.loss_head.normalized, "names": kwargs.get("names", None)}
        # the tower takes pictures [b, 3, H, W]; dummy [b, 1, 1, 1] images and pre-computed [b, E] features pass it by
        if self.image_head is not None and images is not None and images.dim() == 4 and list(images.shape[1:]) != [1, 1, 1]:
            # a frozen tower records no tape; a trainable one follows the caller's grad mode (never re-enabled under no_grad)
            with torch.no_grad() if _frozen(self.image_head) else contextlib.nullcontext():
                image_features = self.image_head(images, **kwargs)
        else:                                   # pre-computed un-normalised features (or dummy images)
            if self.loss_head.normalized and images is not None and images.dim() == 2:
                images = ops.l2_normalize(images)
            image_features = images
        audio_features = self._audio_features(audios, **kwargs)
        return self.loss_head(audio_features, labels, x3=image_features, **kwargs)

    def encode_image(self, images, *args, **kwargs):
        kwargs.pop("device_ids", None)
        return self.image_head(images, **kwargs)

    def report(self, gold_file=None, **kwargs):
        if self.training:
            return self.loss_head.stats(**kwargs) if hasattr(self.loss_head, "stats") else ""
        if not dist.is_initialized() or dist.get_rank() == 0:
            return self.loss_head.report(gold_file=gold_file, **kwargs)
        return ""

    def build(self, **kwargs):
        tunable_params = dict()
        cfg = self.cfg
        loss_kwargs = {k: v for k, v in kwargs.items() if k in ("output_dim",)}
        local_cfg, _, audio_head_sd, _, loss_head_sd = load_checkpoint(cfg, self.echo)
        from_scratch, image_head_sd, text_head_sd, _ = load_clip(None, cfg, self.echo)
        self.image_head = build_image_head(cfg.model.image)
        imagine = cfg.running.get("imagine", True) and cfg.running.get("frame_emb", None) is None
        if cfg.eval:
            if not from_scratch and imagine and image_head_sd is not None:
                self.image_head.copy_state_dict(image_head_sd)
                self.echo("Initialize image encoder from `image_head`.")
            else:
                self.image_head = None
                self.echo("Destory image encoder.")
            self.audio_head = build_audio_head(cfg.model.audio)
            self._init_audio(local_cfg, audio_head_sd, image_head_sd, from_scratch)
            self.text_head = build_text_head(cfg.model.text)
            if text_head_sd is not None:
                n_o, _ = self.text_head.copy_state_dict(text_head_sd)
                self._init_msg("text", "text_head", n_o)
            self.loss_head = build_loss_head(cfg.model.loss, **loss_kwargs)
            try:
                self.loss_head.load_state_dict(loss_head_sd)
            except Exception as e:
                self.echo(f"Failed to load `loss_head` (expected in zero-shot mode) because: {e}")
        else:
            if not from_scratch and not cfg.model.image.from_scratch and image_head_sd is not None:
                self.image_head.copy_state_dict(image_head_sd)
                self.echo("Initialize image encoder from `image_head`.")
            if not imagine:
                self.image_head = None
                self.echo("Destory image encoder.")
            self.audio_head = build_audio_head(cfg.model.audio)
            if not cfg.model.audio.from_scratch:
                if local_cfg is not None and audio_head_sd is not None:
                    self.audio_head.load_state_dict(audio_head_sd)
                    self.echo("Initialize audio encoder from `audio_head`.")
                else:
                    self._init_audio(None, None, image_head_sd, from_scratch)
            self.loss_head = build_loss_head(cfg.model.loss, **loss_kwargs)
            tunable_params = {f"loss_head.{k}": v for k, v in self.loss_head.named_parameters()}
            if not cfg.model.image.freeze and self.image_head is not None:
                tunable_params.update({f"image_head.{k}": v for k, v in self.image_head.named_parameters()})
            elif self.image_head is not None:
                self.echo("Freeze image encoder.")
            self._tunable_audio(tunable_params)
        self.to(self._device())
        return tunable_params
