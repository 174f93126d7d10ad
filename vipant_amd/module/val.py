"""Encoder building blocks with the reference's registry names, constructor signatures, forward
keyword protocol and state_dict keys (cvap/module/val.py), computing through the HIP autograd nodes of
`vipant_amd.ops`.  torch.nn modules appear only as PARAMETER CONTAINERS (same shapes, names and default
initialisation as the reference, so seeds and checkpoints carry over); their forward() is never called.

Differences that are deliberate and MI355X-motivated:
  * activations are batch-first token-major [b, S, D] end to end (`TransformerBackbone.batch_first = True`), so
    MetaHead's two permute copies (clip_head.py:108-110) disappear;
  * the residual stream is fp16 inside a transformer stack (`running.stream_dtype`, the reference's own autocast precision;
    `fp32` selectable) and fp32 at the stack's boundaries; its gradient is bf16; MFMA operands are bf16, accumulation fp32.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from .. import ops
from ..registry import Registry

ENCODER_MODULES_REGISTRY = Registry("ENCODER_MODULES")
ENCODER_MODULES_REGISTRY.__doc__ = "Registry for encoder modules."


def build_encoder_module(cfg, **kwargs):
    """cvap/module/val.py:17-18."""
    return ENCODER_MODULES_REGISTRY.get(cfg.name)(cfg, **kwargs)


def check_tower_width(width, who):
    """A transformer tower's width is 64 H with 3 <= H <= 16 (heads of 64; the widths vipant_layernorm_fwd / _bwd take): anything
    else is refused when the module is built, not by the first launch."""
    if width % 64 != 0 or not 192 <= width <= 1024:
        from ..errors import VipantError
        raise VipantError(f"{who}: width = {width} is not a multiple of 64 from 192 to 1024 (3 to 16 heads of 64: the widths the "
                          "LayerNorm kernels take)")


class LayerNorm(nn.LayerNorm):
    """Parameter container for ln_* (clip/model.py:154-160); the fp32-statistics LayerNorm itself is
    vipant_layernorm_fwd/bwd."""

    def forward(self, x):  # pragma: no cover - guard against accidental eager use
        raise RuntimeError("LayerNorm parameters are consumed by the fused HIP path; do not call the module")


class QuickGELU(nn.Module):
    """Placeholder keeping `mlp.gelu` in the module tree (clip/model.py:163-165); fused into the c_fc epilogue."""

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("QuickGELU is fused into the c_fc contraction epilogue")


class MetaEncoder(nn.Module):
    """cvap/module/val.py:20-32."""

    def __init__(self):
        super().__init__()
        self.position_resolution = None
        self.mask = None

    @property
    def hp(self):
        return []

    @hp.setter
    def hp(self, hp):
        pass


class Miscellanea(MetaEncoder):
    """Positional / class embedding container (cvap/module/val.py:34-51)."""

    def __init__(self, cfg, position_resolution=None, **kwargs):
        super().__init__()
        if position_resolution is not None:
            width = position_resolution[-1]
            self.position_resolution = position_resolution[:-1]
            positions = int(np.prod(self.position_resolution)) + 1
        else:
            self.position_resolution = None
            width, positions = 0, 0
        scale = width ** -0.5 if width > 0 else 0
        self.positional_embedding = nn.Parameter(scale * torch.randn(positions, width))
        self.class_embedding = nn.Parameter(scale * torch.randn(width))

    def initialize_parameters(self):
        pass


@ENCODER_MODULES_REGISTRY.register()
class AddonEncoder(nn.Module):
    """Identity hook between pre-encoder / backbone / post-encoder (cvap/module/val.py:53-61)."""

    def __init__(self, cfg, **kwargs):
        super().__init__()

    def forward(self, x, **kwargs):
        return x


@ENCODER_MODULES_REGISTRY.register()
class CLIPMisc(Miscellanea):
    """cvap/module/val.py:63-92."""

    def replace_modules(self, reference, keep_hp=False):
        self.positional_embedding, self.class_embedding = reference.positional_embedding, reference.class_embedding
        if not keep_hp:
            self.position_resolution = reference.position_resolution

    @property
    def hp(self):
        return [self.position_resolution]

    @hp.setter
    def hp(self, hp):
        (self.position_resolution,) = hp

    @property
    def pos_embedding(self):
        return interp_clip_vp_embedding(self.positional_embedding, self.position_resolution)

    @property
    def cls_embedding(self):
        return self.class_embedding


@ENCODER_MODULES_REGISTRY.register()
class GPTPreEncoder(MetaEncoder):
    """Token embedding + positional table (cvap/module/val.py:94-122); records the EOT index in `.mask`."""

    def __init__(self, cfg, width=512, ctx_len=77, **kwargs):
        super().__init__()
        check_tower_width(width, "GPTPreEncoder")
        self.position_resolution = (ctx_len, width)
        self.token_embedding = nn.Embedding(cfg.vocab_size, width)
        self.initialize_parameters()

    def initialize_parameters(self):
        nn.init.normal_(self.token_embedding.weight, std=0.02)

    @property
    def dtype(self):
        return self.token_embedding.weight.dtype

    def forward(self, x, positional_embedding=None, class_embedding=None, **kwargs):
        b, L = x.shape
        out, self.mask = ops.embed_tokens(x, self.token_embedding.weight, positional_embedding)
        return out.view(b, L, -1)


@ENCODER_MODULES_REGISTRY.register()
class GPTPostEncoder(MetaEncoder):
    """ln_final, EOT gather, text projection (cvap/module/val.py:124-146)."""
    fuses_normalization = True

    def __init__(self, cfg, width=512, embed_dim=512, **kwargs):
        super().__init__()
        check_tower_width(width, "GPTPostEncoder")
        scale = width ** -0.5
        self.ln = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, embed_dim))

    def initialize_parameters(self):
        pass

    def readout_rows(self, mask=None):
        """The one row per item this read-out takes: the end-of-text index the pre-encoder recorded."""
        return mask

    def forward(self, x, positional_embedding=None, class_embedding=None, mask=None, normalized=False, **kwargs):
        b, L, D = x.shape
        if L == 1:          # the stack already returned the read-out rows
            mask = None
        return ops.ReadoutFn.apply(x.reshape(b * L, D), mask, b, L,
                                   *ops.no_tape((self.ln.weight, self.ln.bias, self.proj)), bool(normalized))


def _vit_position_resolution(input_resolution, patch_size, stride):
    """Patch-grid geometry (cvap/module/val.py:148-167)."""
    stride = stride or patch_size
    stride = [stride] * 2 if isinstance(stride, int) else list(stride)
    patch_size = [patch_size] * 2 if isinstance(patch_size, int) else list(patch_size)
    if isinstance(input_resolution, int):
        nrow = ncol = input_resolution // patch_size[0]
    else:
        nrow = (input_resolution[0] - patch_size[0]) // stride[0] + 1
        ncol = (input_resolution[1] - patch_size[1]) // stride[1] + 1
    return stride, nrow * ncol + 1, (nrow, ncol)


def _bilinear_resize(t: torch.Tensor, size) -> torch.Tensor:
    """F.interpolate(mode="bilinear", align_corners=False) for the one-off weight re-gridding at load time
    (cvap/module/val.py:173-189, 545-550).  Init-time only, never on the training path; runs on the tensor's
    device through torch (weight surgery is host logic)."""
    return torch.nn.functional.interpolate(t, tuple(int(s) for s in size), mode="bilinear", align_corners=False)


def interp_conv_weight_channel(conv_weight, input_shape):
    """cvap/module/val.py:169-180."""
    if conv_weight.shape[1] != input_shape[1]:
        shape = (conv_weight.shape[0], input_shape[1])
        conv_weight = _bilinear_resize(conv_weight.permute(2, 3, 0, 1), shape).permute(2, 3, 0, 1)
    return conv_weight


def interp_conv_weight_spatial(conv_weight, patch_shape):
    """cvap/module/val.py:182-190."""
    if tuple(conv_weight.shape[-2:]) != tuple(patch_shape):
        conv_weight = _bilinear_resize(conv_weight, patch_shape)
    return conv_weight


def interp_clip_vp_embedding(old_pos_emb, pos_resolution, old_pos_resolution=None, bop=1):
    """Re-grid a visual positional table (cvap/module/val.py:524-556); identity when sizes already agree,
    which is always the case on the training path."""
    num_pos, pos_dim = old_pos_emb.shape[-2:]
    if int(np.prod(pos_resolution)) + 1 == num_pos:
        return old_pos_emb
    if old_pos_resolution is None:
        h = w = int(np.sqrt(num_pos - bop))
    else:
        h, w = old_pos_resolution
    grid = old_pos_emb[bop:].reshape(-1, h, w, pos_dim).permute(0, 3, 1, 2)
    if tuple(grid.shape[-2:]) == tuple(pos_resolution):
        return old_pos_emb
    new = _bilinear_resize(grid, pos_resolution).permute(0, 2, 3, 1).flatten(1, 2)
    return torch.cat((old_pos_emb[:bop], new.view(-1, pos_dim)), dim=0)


@ENCODER_MODULES_REGISTRY.register()
class ViTPreEncoder(MetaEncoder):
    """Patch conv + cls token + positional table + ln_pre (cvap/module/val.py:192-259)."""

    def __init__(self, cfg, width=768, resolution=224, **kwargs):
        super().__init__()
        check_tower_width(width, "ViTPreEncoder")
        self.stride, _, self.position_resolution = _vit_position_resolution(resolution, cfg.patch_size, cfg.stride)
        self.position_resolution += (width,)
        self.conv1 = nn.Conv2d(in_channels=cfg.in_channels, out_channels=width, kernel_size=cfg.patch_size,
                               stride=self.stride, bias=False)
        self.patch_size = self.conv1.weight.shape[-2:]
        self.ln = LayerNorm(width)
        # `+model.<head>.pre_encoder.patchout.keep=0.5` (or `.time=` / `.freq=`; the key is in no config group): training steps embed a
        # random subset of every clip's patches (ops.PatchoutEmbedFn); evaluation and no_grad calls always see every patch
        po = cfg.get("patchout", None) if hasattr(cfg, "get") else getattr(cfg, "patchout", None)
        self.patchout = None
        if po is not None:
            po = dict(po) if isinstance(po, dict) else dict(vars(po))
            unknown = set(po) - {"keep", "time", "freq"}
            if unknown or not po:
                from ..errors import VipantError
                raise VipantError(f"ViTPreEncoder: patchout takes `keep`, or `time` / `freq`; got {sorted(po)}")
            nrow, ncol = self.position_resolution[:2]
            ops.draw_patchout(1, nrow, ncol, **po)          # a rule that leaves no patch is refused here, when the tower is built
            self.patchout = po
        self._patchout_seed = 0
        self._patchout_generator = None

    def seed_patchout(self, seed, rank=0):
        """The module's own generator for the kept-patch lists: `seed` of the run and the replica's rank, so replicas draw different
        lists (Monitor._configure)."""
        self._patchout_seed = int(seed) + 4409 + 1000 * max(int(rank), 0)
        self._patchout_generator = None

    def draw_keep(self, b, nrow, ncol):
        if self._patchout_generator is None:
            self._patchout_generator = torch.Generator().manual_seed(self._patchout_seed)
        return ops.draw_patchout(b, nrow, ncol, generator=self._patchout_generator, **self.patchout)

    def initialize_parameters(self):
        pass

    def replace_modules(self, reference, keep_hp=False):
        self.conv1, self.ln = reference.conv1, reference.ln
        if not keep_hp:
            self.stride, self.patch_size, self.position_resolution = \
                reference.stride, reference.patch_size, reference.position_resolution

    @property
    def hp(self):
        return [self.stride, self.patch_size, self.position_resolution]

    @hp.setter
    def hp(self, hp):
        (self.stride, self.patch_size, self.position_resolution) = hp

    @property
    def dtype(self):
        return self.conv1.weight.dtype

    def forward(self, x, positional_embedding=None, class_embedding=None, keep=None, **kwargs):
        """`keep` (int32 [b, k], ops.draw_patchout): an explicit list of kept patches for a patchout step (tests); None: drawn."""
        assert x.dim() == 4, f"expect 4d `x` but get x.dim == {x.dim()}"
        w = self.conv1.weight
        if x.shape[1] != 3:
            w = interp_conv_weight_spatial(w, self.patch_size)       # no-op unless the kernel was re-gridded
        b = x.shape[0]
        if self.patchout is not None and self.training and torch.is_grad_enabled():
            if keep is None:
                ph, pw = w.shape[-2:]
                keep = self.draw_keep(b, (x.shape[2] - ph) // self.stride[0] + 1, (x.shape[3] - pw) // self.stride[1] + 1)
            out = ops.PatchoutEmbedFn.apply(x.to(torch.float32), w, class_embedding, positional_embedding,
                                            self.ln.weight, self.ln.bias, tuple(self.stride), keep)
            return out.view(b, -1, out.shape[-1])
        out = ops.PatchEmbedFn.apply(x.to(torch.float32), w, class_embedding, positional_embedding,
                                     self.ln.weight, self.ln.bias, tuple(self.stride))
        return out.view(b, -1, out.shape[-1])


@ENCODER_MODULES_REGISTRY.register()
class ViTPostEncoder(MetaEncoder):
    """ln_post(cls row) @ proj (cvap/module/val.py:261-290)."""
    fuses_normalization = True

    def __init__(self, cfg, width=768, embed_dim=512, **kwargs):
        super().__init__()
        check_tower_width(width, "ViTPostEncoder")
        scale = width ** -0.5
        self.ln = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, embed_dim))

    def initialize_parameters(self):
        pass

    def readout_rows(self, mask=None):
        """The one row per item this read-out takes: the class token."""
        return "first"

    def forward(self, x, positional_embedding=None, class_embedding=None, position_resolution=None,
                require_feature=False, normalized=False, **kwargs):
        if require_feature:
            raise NotImplementedError("require_feature (encoder-decoder captioning) is outside the contrastive path")
        b, S, D = x.shape
        return ops.ReadoutFn.apply(x.reshape(b * S, D), None, b, S,
                                   *ops.no_tape((self.ln.weight, self.ln.bias, self.proj)), bool(normalized))


class ResidualAttentionBlock(nn.Module):
    """Parameter layout of one pre-LN block (cvap/module/val.py:496-522): attn (packed in_proj + out_proj),
    ln_1, mlp.{c_fc, gelu, c_proj}, ln_2.  Compute lives in ops.BackboneFn."""

    def __init__(self, d_model: int, n_head: int, attn_mask=None, skip_attn_mask: bool = True):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([
            ("c_fc", nn.Linear(d_model, d_model * 4)),
            ("gelu", QuickGELU()),
            ("c_proj", nn.Linear(d_model * 4, d_model)),
        ]))
        self.ln_2 = LayerNorm(d_model)
        self.skip_attn_mask = skip_attn_mask
        self.causal = (not skip_attn_mask) and attn_mask is not None

    def flat_params(self):
        sd = dict(self.named_parameters())
        return [sd[n] for n in ops.BLOCK_PARAM_NAMES]

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("blocks are executed by TransformerBackbone through ops.BackboneFn")


@ENCODER_MODULES_REGISTRY.register()
class TransformerBackbone(MetaEncoder):
    """cvap/module/val.py:468-494.  heads = width // 64; causal mask iff ctx_len is set and not skip_attn_mask."""

    def __init__(self, cfg, width=512, ctx_len=77, **kwargs):
        super().__init__()
        self.batch_first = True     # token-major batch-first kernels: MetaHead skips its permutes
        self.ctx_len = ctx_len
        check_tower_width(width, "TransformerBackbone")
        self.width = width
        heads = width // 64
        attn_mask = self.build_attention_mask()
        self.resblocks = nn.Sequential(*[
            ResidualAttentionBlock(width, heads, attn_mask, cfg.skip_attn_mask) for _ in range(cfg.layers)
        ])
        self.causal = (not cfg.skip_attn_mask) and attn_mask is not None
        self.grad_sync = None       # set by vipant_amd.parallel for data-parallel replicas
        self.recompute_mlp = False  # `running.recompute_mlp`: do not keep the [M, 4D] MLP activations for the backward
        self.fp8 = False            # `running.fp8_gemm`: e4m3 operands in the NT contractions of the trainable blocks (configs[4])
        self.stream_f16 = True      # `running.stream_dtype` (fp16 | fp32): residual stream inside the stack in the reference's autocast precision
        self.last_block_rows = True     # `running.last_block_rows`: honour `rows=` (the last block on the read-out rows only; exact)

    @property
    def fp8(self):
        return self._fp8

    @fp8.setter
    def fp8(self, on):
        """The e4m3 forms of the LayerNorm outputs exist in the kernels for the multiples of 256 only: an e4m3 tower of another
        width is refused here, when the tower is configured."""
        if on and self.width not in (256, 512, 768, 1024):
            from ..errors import VipantError
            raise VipantError(f"running.fp8_gemm=True: a tower of width {self.width} has no e4m3 kernels; the widths with e4m3 towers "
                              "are 256, 512, 768 and 1024")
        if on and getattr(self, "patchout", False):       # MetaHead marks the stack of a tower whose pre-encoder has `patchout`
            from ..errors import VipantError
            raise VipantError("running.fp8_gemm=True: a tower with `pre_encoder.patchout` is refused: e4m3 plans over the kept "
                              "rows are not supported; drop one of the two keys")
        self._fp8 = bool(on)

    def build_attention_mask(self):
        """Marker only: the -inf upper-triangular mask (val.py:484-491) is applied inside the attention kernel."""
        return None if self.ctx_len is None else "causal"

    def forward(self, x, rows=None, **kwargs):
        """`rows` (None | "first" | int64 [b]): the one row per item the caller is going to read (MetaHead asks its post-encoder):
        the stack then returns [b, 1, D] -- those rows -- and evaluates its last block on them alone (ops.BackboneFn)."""
        b, S, D = x.shape
        if self.causal and S > self.ctx_len:
            raise ValueError(f"sequence length {S} exceeds ctx_len {self.ctx_len}")
        params = [p for blk in self.resblocks for p in blk.flat_params()]
        if not self.last_block_rows or len(params) == 0:
            rows = None
        out = ops.BackboneFn.apply(x.reshape(b * S, D), b, S, self.causal, self.grad_sync, self.recompute_mlp, self.fp8,
                                   self.stream_f16, rows, *ops.no_tape(params))
        return out.view(b, S if rows is None else 1, D)


# ------------------------------------------------------------------------------------------ CLIP ModifiedResNet towers
# Forward only (frozen image tower of VA pre-training, evaluation of a ResNet audio head): the kernels of csrc/resnet.hip through
# vipant_amd/resnet.py.  nn.Conv2d / nn.BatchNorm2d / nn.Linear are parameter containers with the reference's names, shapes and
# default initialisation; `module.training` selects the BatchNorm mode as in torch (the ResNet section).

RESNET_TRAINABLE = ("a trainable ResNet tower is not supported: the ModifiedResNet modules (ResNetPreEncoder / ResNetBackbone / "
                    "ResNetPostEncoder) have a forward pass only -- freeze the head (model.image.freeze=True / model.audio.freeze=True) "
                    "or run it under torch.no_grad().  The backward pass is opt-in: +model.image.resnet_backward=True / "
                    "+model.audio.resnet_backward=True")


def _refuse_trainable_resnet(module):
    """Without the head's `resnet_backward` key the convolution, BatchNorm2d, the average pool and the attention pool run without a
    tape: a call that autograd would record is an error, not a silently constant tower."""
    if getattr(module, "resnet_backward", False):
        return
    if torch.is_grad_enabled() and any(p.requires_grad for p in module.parameters()):
        from ..errors import VipantError
        raise VipantError(RESNET_TRAINABLE)


def set_resnet_backward(head, enabled: bool):
    """Carry the head-level key `resnet_backward` (absent = False) to the ModifiedResNet modules of `head`."""
    for m in head.modules():
        if isinstance(m, (ResNetPreEncoder, ResNetBackbone, ResNetPostEncoder, Bottleneck)):
            m.resnet_backward = bool(enabled)


def is_resnet_head(head) -> bool:
    return any(isinstance(m, (ResNetPreEncoder, ResNetBackbone, ResNetPostEncoder)) for m in head.modules())


def _resnet_position_resolution(input_resolution, patch_size=32, stride=None):
    """cvap/module/val.py:292-308."""
    stride = stride or patch_size
    stride = [stride] * 2 if isinstance(stride, int) else list(stride)
    if isinstance(input_resolution, int):
        nrow = ncol = input_resolution // patch_size
    else:
        nrow, ncol = input_resolution[0] // stride[0], input_resolution[1] // stride[1]
    return stride, nrow * ncol + 1, (nrow, ncol)


class Bottleneck(nn.Module):
    """Parameter layout of clip/model.py:11-39 (conv1/bn1, conv2/bn2, avgpool, conv3/bn3, downsample.{-1, 0, 1}); the compute is
    vipant_amd.resnet.bottleneck."""
    expansion = 4
    resnet_backward = False      # set_resnet_backward: record an autograd tape (vipant_amd.resnet.ConvBnFn)

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.avgpool = nn.AvgPool2d(stride) if stride > 1 else nn.Identity()
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        self.stride = stride
        if stride > 1 or inplanes != planes * Bottleneck.expansion:
            self.downsample = nn.Sequential(OrderedDict([
                ("-1", nn.AvgPool2d(stride)),
                ("0", nn.Conv2d(inplanes, planes * self.expansion, 1, stride=1, bias=False)),
                ("1", nn.BatchNorm2d(planes * self.expansion)),
            ]))

    def forward(self, x):
        from .. import resnet
        return resnet.bottleneck(self, x, backward=self.resnet_backward)


@ENCODER_MODULES_REGISTRY.register()
class ResNetPreEncoder(MetaEncoder):
    """The three-convolution stem and its average pool (cvap/module/val.py:310-355): fp32 NCHW in, bf16 NHWC [n, H/4, W/4, width] out."""
    resnet_backward = False

    def __init__(self, cfg, width=64, **kwargs):
        super().__init__()
        self.conv1 = nn.Conv2d(cfg.in_channels, width // 2, kernel_size=3, stride=2, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(width // 2)
        self.conv2 = nn.Conv2d(width // 2, width // 2, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(width // 2)
        self.conv3 = nn.Conv2d(width // 2, width, kernel_size=3, padding=1, bias=False)
        self.bn3 = nn.BatchNorm2d(width)
        self.avgpool = nn.AvgPool2d(2)
        self.relu = nn.ReLU(inplace=True)
        self.initialize_parameters()

    def initialize_parameters(self):
        pass

    @property
    def dtype(self):
        return self.conv1.weight.dtype

    def forward(self, x, positional_embedding=None, class_embedding=None, **kwargs):
        from .. import resnet
        assert x.dim() == 4, f"expect 4d `x` but get x.dim == {x.dim()}"
        _refuse_trainable_resnet(self)
        # an input with another channel count than 3 meets the channel mean of the weight (val.py:340-348); the packed copy is
        # remade when the weight changes
        mean = x.shape[1] != 3
        if mean and x.shape[1] != 1:
            raise ValueError(f"the ResNet stem takes 3 channels, or 1 with the channel-mean weight; got {x.shape[1]}")
        if not mean and self.conv1.weight.shape[1] != 3:
            raise ValueError(f"a 3-channel input needs a 3-channel conv1, which has {self.conv1.weight.shape[1]}")
        bwd = self.resnet_backward
        if bwd and torch.is_grad_enabled() and x.requires_grad:
            from ..errors import VipantError
            raise VipantError("the ResNet stem's input is the data: a gradient with respect to it (the data gradient of the stride-2 "
                              "conv1) is not implemented")
        x = resnet.nchw_to_nhwc(x.to(torch.float32))
        x = resnet.conv_bn(x, self.conv1, self.bn1, relu=True, channel_mean=mean, backward=bwd)
        x = resnet.conv_bn(x, self.conv2, self.bn2, relu=True, backward=bwd)
        return resnet.conv_bn(x, self.conv3, self.bn3, relu=True, pool=2, backward=bwd)


@ENCODER_MODULES_REGISTRY.register()
class ResNetPostEncoder(MetaEncoder):
    """The attention pool (cvap/module/val.py:357-424; clip/model.py:57-91): bf16 NHWC [n, H, W, 32 width] -> fp32 [n, embed_dim]."""
    resnet_backward = False

    def __init__(self, cfg, width=64, embed_dim=None, resolution=224, **kwargs):
        super().__init__()
        width = width * 32
        self.num_heads = width // 64
        _, _, self.position_resolution = _resnet_position_resolution(resolution)
        self.position_resolution += (width,)
        self.k_proj = nn.Linear(width, width)
        self.q_proj = nn.Linear(width, width)
        self.v_proj = nn.Linear(width, width)
        self.c_proj = nn.Linear(width, embed_dim or width)
        self.initialize_parameters()

    def initialize_parameters(self):
        std = self.c_proj.in_features ** -0.5
        for lin in (self.q_proj, self.k_proj, self.v_proj, self.c_proj):
            nn.init.normal_(lin.weight, std=std)

    def replace_modules(self, reference, keep_hp=False):
        self.k_proj, self.q_proj, self.v_proj, self.c_proj = reference.k_proj, reference.q_proj, reference.v_proj, reference.c_proj
        if not keep_hp:
            self.position_resolution = reference.position_resolution

    @property
    def hp(self):
        return [self.position_resolution]

    @hp.setter
    def hp(self, hp):
        (self.position_resolution,) = hp

    def forward(self, x, positional_embedding=None, class_embedding=None, **kwargs):
        from .. import resnet
        _refuse_trainable_resnet(self)
        return resnet.attention_pool(self, x, positional_embedding, backward=self.resnet_backward)


@ENCODER_MODULES_REGISTRY.register()
class ResNetBackbone(MetaEncoder):
    """layer1 .. layer4 of Bottleneck blocks (cvap/module/val.py:426-466); bn3.weight starts at zero in every block."""
    resnet_backward = False

    def __init__(self, cfg, width=64, **kwargs):
        super().__init__()
        self.batch_first = True
        layers = cfg.layers
        self._inplanes = width
        self.layer1 = self._make_layer(width, layers[0])
        self.layer2 = self._make_layer(width * 2, layers[1], stride=2)
        self.layer3 = self._make_layer(width * 4, layers[2], stride=2)
        self.layer4 = self._make_layer(width * 8, layers[3], stride=2)
        self.grad_sync = None       # (the trainer hands every backbone its replica reduction; a frozen tower has nothing to reduce)
        self.initialize_parameters()

    def _make_layer(self, planes, blocks, stride=1):
        layers = [Bottleneck(self._inplanes, planes, stride)]
        self._inplanes = planes * Bottleneck.expansion
        for _ in range(1, blocks):
            layers.append(Bottleneck(self._inplanes, planes))
        return nn.Sequential(*layers)

    def initialize_parameters(self):
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for name, param in layer.named_parameters():
                if name.endswith("bn3.weight"):
                    nn.init.zeros_(param)

    @property
    def dtype(self):
        return self.layer1[0].conv1.weight.dtype

    def forward(self, x, **kwargs):
        _refuse_trainable_resnet(self)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            x = layer(x)
        return x
