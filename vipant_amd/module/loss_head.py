"""Loss heads with the reference's registry / forward contract (cvap/module/decoder/loss_head.py).

Training path: `CELossHead.forward` = symmetric InfoNCE through the fused HIP kernels (ops.InfoNCEFn); in a
replica group the features are first all-gathered so every rank scores the GLOBAL batch -- the semantics of
the reference's dp mode, where the loss head sees the gathered batch (cvap/model/cvalp.py:41-61).
Eval path: `infer` caches normalised features on the device, `report` ranks them with the fused retrieval kernels.
"""
from __future__ import annotations

import copy
import json
import logging
from collections import defaultdict

import numpy as np
import torch
import torch.distributed as dist
from torch import nn

from .. import ops, parallel
from .._ffi import VipantError
from ..registry import Registry

LOSS_HEADS_REGISTRY = Registry("LOSS_HEADS")


def build_loss_head(cfg, **kwargs):
    return LOSS_HEADS_REGISTRY.get(cfg.name)(cfg, **kwargs)


class LossHead(nn.Module):
    """cvap/module/decoder/loss_head.py:25-244: feature cache (`infer`) and the retrieval report.

    The reference sorts every row of `x1s @ x2s.t()` and looks up the gold column; here the ranks come from
    `ops.retrieval_ranks` (fused similarity tiles + counting on the GPU, nothing N x N is stored).  What is left on
    the host is the formatting of a few counters, done in the reference's own dtypes so the strings agree."""

    def __init__(self):
        super().__init__()
        self.reduce = False
        self.normalized = True

    def copy_state_dict(self, state_dict):
        pass

    def infer(self, x1, x2, *args, **kwargs):
        if not hasattr(self, "x1s") or not hasattr(self, "x2s") or not hasattr(self, "ids"):
            self.x1s, self.x2s, self.ids = [], [], []
        if not kwargs.get("normalized", False):
            x1, x2 = ops.l2_normalize(x1.detach().float()), ops.l2_normalize(x2.detach().float())
        self.x1s.append(x1.detach().float())
        self.x2s.append(x2.detach().float())
        names = kwargs.get("names", None)
        if names is not None:
            self.ids.extend(names)
        return None

    @staticmethod
    def _gold_cluster(gold_file, nsample, verbose=False):
        """loss_head.py:48-66: class name ("labels" joined by blanks) <-> sample ids, first `nsample` records."""
        sample_by_classname, classname_by_sample = defaultdict(list), defaultdict(str)
        with open(gold_file, "r") as fr:
            for iline, line in enumerate(fr):
                if iline + 1 > nsample:
                    break
                record = json.loads(line)
                key = " ".join(record["labels"])
                sample_by_classname[key].append(record["id"])
                classname_by_sample[record["id"]] = key
        return sample_by_classname, classname_by_sample

    @staticmethod
    def retrieval_metrics(ranks, nsample=None, msg=""):
        """loss_head.py:68-78; `ranks` is a float32 vector as in the reference (median = lower median)."""
        ranks = torch.as_tensor(ranks).float().cpu()
        nsample = nsample or ranks.shape[0]
        hit = lambda k: int((ranks < k).sum()) / nsample * 100.
        med, avg = ranks.median() + 1, ranks.mean() + 1
        return (f"{msg}: R@1 {hit(1):2.2f} R5 {hit(5):2.2f} R10 {hit(10):2.2f} R50 {hit(50):2.2f} "
                f"MED {med:2.2f} AVG {avg:2.2f}")

    @staticmethod
    def _one_v_k_ranks(x1s, x2s, k=5):
        """ranks of the k captions of every clip (x1 -> x2, [n1, k]) and of every caption's clip (x2 -> x1, [n1 * k])."""
        n1 = x1s.shape[0]
        gold12 = torch.arange(n1 * k, dtype=torch.int32).reshape(n1, k)
        gold21 = torch.arange(n1, dtype=torch.int32).repeat_interleave(k)
        return ops.retrieval_ranks(x1s, x2s, gold12).cpu(), ops.retrieval_ranks(x2s, x1s, gold21).cpu()

    @staticmethod
    def retrieval_eval(x1s, x2s, k=5, _ranks=None):
        """loss_head.py:80-107: best-caption rank per clip and clip rank per caption."""
        r12, r21 = _ranks if _ranks is not None else LossHead._one_v_k_ranks(x1s, x2s, k)
        msg_12 = LossHead.retrieval_metrics(r12.min(-1)[0], msg="A->T")
        msg_21 = LossHead.retrieval_metrics(r21, msg="T->A")
        return f"{msg_12}\n{msg_21}"

    def _class_stats(self, top1, sample_by_classname, classname_by_sample, nsample, msg, k=1):
        """loss_head.py:176-232 (topk_overlap + pnr at k = 1): precision / recall of the nearest neighbour by class."""
        stats = defaultdict(dict)
        for idx, neighbor in enumerate(top1):
            sample = self.ids[idx]
            classname = classname_by_sample[sample]
            true_neighbors = sample_by_classname[classname]
            sample_stat = stats.get(classname, {})
            this_stat = sample_stat.get(sample, [0] * 2)
            if self.ids[neighbor] in true_neighbors:
                this_stat[0] += 1
            sample_stat[sample] = this_stat
            stats[classname] = sample_stat
        p = r = p_cls = r_cls = 0.
        nclass = len(sample_by_classname)
        for classname, class_stats in stats.items():
            nrelevant = len(sample_by_classname[classname])
            pc = rc = 0
            for sample, (tp, _) in class_stats.items():
                p += tp / k; r += tp / nrelevant
                pc += tp / k; rc += tp / nrelevant
            p_cls += pc / nrelevant
            r_cls += rc / nrelevant
        p, r = (p / nsample) * 100, (r / nsample) * 100
        p_cls, r_cls = (p_cls / nclass) * 100, (r_cls / nclass) * 100
        return f"{msg}: P@{k} {p:2.2f} R@{k} {r:2.2f} mAP {p_cls:2.2f} mAR {r_cls:2.2f}"

    def report(self, gold_file=None):
        x1s, x2s = torch.cat(self.x1s), torch.cat(self.x2s)
        n1, n2 = x1s.shape[0], x2s.shape[0]
        ref_metric = ""
        top12 = top21 = None
        if n1 == n2:
            gold = torch.arange(n1, dtype=torch.int32)
            r12, top12 = ops.retrieval_ranks(x1s, x2s, gold, want_top1=True)
            r21, top21 = ops.retrieval_ranks(x2s, x1s, gold, want_top1=True)
            pct = lambda r, k: int((r < k).sum()) / n1 * 100.
            p_12 = f"I->A: t1 = {pct(r12, 1):2.2f} t5 = {pct(r12, 5):2.2f}"
            p_21 = f"A->I: t1 = {pct(r21, 1):2.2f} t5 = {pct(r21, 5):2.2f}"
        elif n1 * 5 == n2:   # 1 clip vs 5 captions (loss_head.py:135-168)
            r12, r21 = self._one_v_k_ranks(x1s, x2s, 5)
            t1 = (r12 < 1).sum(-1).sum() / (1 * n1) * 100.     # float32 tensors, as in the reference
            t5 = (r12 < 5).sum(-1).sum() / (5 * n1) * 100.
            mean = r12.min(-1)[0].float().mean() + 1
            p_12 = f"A->T: t1 = {t1:2.2f} t5 = {t5:2.2f} mR = {mean:2.2f}"
            t1 = int((r21 < 1).sum()) / n2 * 100.
            t5 = int((r21 < 5).sum()) / n2 * 100.
            mean = r21.float().mean() + 1
            p_21 = f"T->A: t1 = {t1:2.2f} t5 = {t5:2.2f} mR = {mean:2.2f}"
            ref_metric = self.retrieval_eval(x1s, x2s, _ranks=(r12, r21))
            gold_file = None
        else:
            p_12, p_21 = f"{x1s.shape}x{x2s.shape}", "-"
            gold_file = None
        msg_12 = msg_21 = ""
        if gold_file is not None:
            by_class, by_sample = self._gold_cluster(gold_file, n1)
            msg_12 = self._class_stats(top12.tolist(), by_class, by_sample, n1, "I->A")
            msg_21 = self._class_stats(top21.tolist(), by_class, by_sample, n1, "A->I")
        del self.x1s, self.x2s, self.ids
        msg = "" if msg_12 == msg_21 == "" else f"\n{msg_12} {msg_21}\n"
        ref = "" if ref_metric == "" else f"\nREFERENCE\n{ref_metric}"
        return f"{msg}{p_12} {p_21} @ {n1}{ref}"


def zero_shot_report(audios, labels, text, label_map=None) -> str:
    """Zero-shot classification report: the `text is not None` branch of ClassificationHead.report
    (cvap/module/decoder/loss_head.py:371-407), as used by cvap/monitor/esc50_clf.py:260-325.

    audios [n, E] audio features, text [c, E] one feature per class prompt, labels int [n]; the prediction is the
    arg-max prompt (mapped through `label_map` when prompts and labels use different ids).  The reference sorts all of
    `audios @ text.t()`; here the arg-max comes from the fused retrieval kernel (`top1`), nothing n x c is stored."""
    audios, text = audios.detach().float().contiguous(), text.detach().float().contiguous()
    n = audios.shape[0]
    gold = torch.zeros((n,), dtype=torch.int32)
    _, top1 = ops.retrieval_ranks(audios, text, gold, want_top1=True)
    predictions = top1.long()
    if isinstance(label_map, dict):
        predictions = torch.tensor([label_map[x] for x in predictions.tolist()], device=predictions.device)
    labels = torch.as_tensor(labels, device=predictions.device).long()
    precision = (predictions == labels).sum() / n * 100.      # float32 tensor, as in the reference
    return f"A->T: p1 = {precision:2.2f} @ {n}"


@LOSS_HEADS_REGISTRY.register()
class CELossHead(LossHead):
    """Symmetric InfoNCE with a learnable temperature (cvap/module/decoder/loss_head.py:246-284)."""

    def __init__(self, cfg, **kwargs):
        super().__init__()
        self.logit_scale = (nn.Parameter(torch.ones([]) * np.log(1 / 0.07)) if cfg.scaling
                            else torch.ones([], requires_grad=False) * np.log(1 / 1))
        self.scale_max = cfg.scale_max or float("inf")
        self.reduce = False
        # replica groups: "global" = all-gather features, B-way negatives (reference dp semantics);
        # "local" = per-rank negatives, objective = mean over ranks of the per-rank loss (what the reference's ddp mode
        # would compute): every gradient leaves the kernel scaled by 1/world and the replicas SUM-reduce
        self.negatives = kwargs.get("negatives", "global")

    def copy_state_dict(self, state_dict):
        key = "logit_scale"
        new_dict = self.state_dict()
        if key in new_dict and key in state_dict:
            new_dict.update({key: state_dict[key]})
        self.load_state_dict(new_dict)

    def forward(self, x1, x2, *args, **kwargs):
        if not self.training:
            if not dist.is_initialized() or dist.get_rank() == 0:
                return self.infer(x1, x2, *args, **kwargs)
            return None
        if not kwargs.get("normalized", False):
            x1, x2 = ops.L2NormFn.apply(x1), ops.L2NormFn.apply(x2)
        scale_max = 0.0 if self.scale_max == float("inf") else float(self.scale_max)
        ls = self.logit_scale if isinstance(self.logit_scale, nn.Parameter) else self.logit_scale.to(x1.device)
        b = x1.shape[0]
        if parallel.active() and self.negatives == "global":
            x1g, x2g = parallel.all_gather_features(x1, x2)
            return ops.InfoNCEFn.apply(x1g, x2g, ls, scale_max, parallel.rank() * b, b, 1.0)
        return ops.InfoNCEFn.apply(x1, x2, ls, scale_max, 0, b, 1.0 / parallel.world_size() if parallel.active() else 1.0)


@LOSS_HEADS_REGISTRY.register()
class VALCELossHead(LossHead):
    """Sum of pairwise InfoNCE heads over {vision, audio, language} (loss_head.py:421-495); the AT script
    enables only `al`."""

    def __init__(self, cfg, **kwargs):
        super().__init__()
        self.loss_head_va = self.loss_head_lv = self.loss_head_al = None
        self._total_loss = {}
        if cfg.va:
            self.loss_head_va = CELossHead(cfg, **kwargs)
            self._total_loss.update({"va": 0.})
        if cfg.lv:
            self.loss_head_lv = CELossHead(cfg, **kwargs)
            self._total_loss.update({"lv": 0.})
        if cfg.al:
            self.loss_head_al = CELossHead(cfg, **kwargs)
            self._total_loss.update({"al": 0.})

    def copy_state_dict(self, state_dict):
        pass

    def _pairs(self, x1, x2, x3):
        return (("va", self.loss_head_va, x1, x2), ("lv", self.loss_head_lv, x1, x3), ("al", self.loss_head_al, x2, x3))

    def infer(self, x1, x2, x3, *args, **kwargs):
        for _, head, a, b in self._pairs(x1, x2, x3):
            if a is not None and b is not None and head is not None:
                head.infer(a, b, *args, **kwargs)
        return 0.0

    def stats(self, nstep=1, **kwargs):
        return " ".join(f"{k} {float(v) / nstep:.3f}" for k, v in self._total_loss.items())

    def report(self, gold_file=None):
        out = []
        for tag, head in (("VA", self.loss_head_va), ("LV", self.loss_head_lv), ("AL", self.loss_head_al)):
            if head is not None:
                out.append(f"{tag}: " + head.report(gold_file))
        return "\n" + "\n".join(out).strip()

    def forward(self, x1, x2, x3, *args, **kwargs):
        """v: x1; a: x2; l: x3."""
        if not self.training:
            if not dist.is_initialized() or dist.get_rank() == 0:
                return self.infer(x1, x2, x3, *args, **kwargs)
            return None
        loss = 0.0
        for key, head, a, b in self._pairs(x1, x2, x3):
            if a is not None and b is not None and head is not None:
                term = head(a, b, *args, **kwargs)
                self._total_loss[key] += term.detach()
                loss = loss + term
        return loss


@LOSS_HEADS_REGISTRY.register()
class VACELossHead(LossHead):
    """Up to five weighted InfoNCE terms over {prime image features, two image views, two audio views}
    (cvap/module/decoder/loss_head.py:498-598).  Sub-heads `loss_head_{vp,ap,va,vv,aa}` are CELossHeads as in the reference (its
    state dict loads strictly); they own the temperatures and the eval caches.  The training forward is ONE ops.InfoNCEMultiFn node
    over the live operands and pairs: every operand is prepared once and its gradient is summed over its pairs inside the kernel;
    under replicas with global negatives all live operands travel in one all-gather."""

    # (key, first argument, second argument) of each sub-head's call, in the reference's order; operands by forward()'s names
    PAIRS = (("vp", "images_v1", "images"), ("ap", "audios_v1", "images"), ("va", "images_v1", "audios_v1"),
             ("vv", "images_v1", "images_v2"), ("aa", "audios_v1", "audios_v2"))

    def __init__(self, cfg, **kwargs):
        super().__init__()
        self._total_loss = {}
        for key, _, _ in self.PAIRS:
            on = bool(getattr(cfg, key))
            setattr(self, f"loss_head_{key}", CELossHead(cfg, **kwargs) if on else None)
            if on:
                self._total_loss[key] = 0.
        self.vp_w, self.ap_w, self.va_w, self.vv_w, self.aa_w = cfg.vp_w, cfg.ap_w, cfg.va_w, cfg.vv_w, cfg.aa_w
        self.negatives = kwargs.get("negatives", "global")

    def copy_state_dict(self, state_dict):
        pass

    def _live(self, operands):
        """[(key, sub-head, name of x1, name of x2)] of the terms whose head exists and whose two operands are given."""
        return [(key, getattr(self, f"loss_head_{key}"), a, b) for key, a, b in self.PAIRS
                if getattr(self, f"loss_head_{key}") is not None and operands[a] is not None and operands[b] is not None]

    def infer(self, images, images_v1, audios_v1, images_v2=None, audios_v2=None, *args, **kwargs):
        operands = dict(images=images, images_v1=images_v1, audios_v1=audios_v1, images_v2=images_v2, audios_v2=audios_v2)
        for _, head, a, b in self._live(operands):
            head.infer(operands[a], operands[b], *args, **kwargs)
        return 0.

    def stats(self, nstep=1, **kwargs):
        return " ".join(f"{k} {float(v) / nstep:.3f}" for k, v in self._total_loss.items())

    def report(self, gold_file=None):
        out = []
        for key, _, _ in self.PAIRS:
            head = getattr(self, f"loss_head_{key}")
            if head is not None and hasattr(head, "x1s"):
                out.append(f"{key.upper()}: " + head.report(gold_file))
        return "\n" + "\n".join(out).strip()

    def forward(self, images, images_v1, audios_v1, images_v2=None, audios_v2=None, *args, **kwargs):
        if not self.training:
            if not dist.is_initialized() or dist.get_rank() == 0:
                return self.infer(images, images_v1, audios_v1, images_v2=images_v2, audios_v2=audios_v2, *args, **kwargs)
            return None
        operands = dict(images=images, images_v1=images_v1, audios_v1=audios_v1, images_v2=images_v2, audios_v2=audios_v2)
        live = self._live(operands)
        if not live:
            return 0.
        names = [n for n in operands if any(n in (a, b) for _, _, a, b in live)]
        xs = [operands[n] for n in names]
        if not kwargs.get("normalized", False):
            xs = [ops.L2NormFn.apply(x) for x in xs]
        b = xs[0].shape[0]
        row0, grad_scale = 0, 1.0
        if parallel.active() and self.negatives == "global":
            xs = parallel.all_gather_features(*xs)
            row0 = parallel.rank() * b
        elif parallel.active():
            grad_scale = 1.0 / parallel.world_size()
        heads = [head for _, head, _, _ in live]
        scales = [h.logit_scale if isinstance(h.logit_scale, nn.Parameter) else h.logit_scale.to(xs[0].device) for h in heads]
        meta = ops.InfoNCEMultiMeta([(names.index(a), names.index(b)) for _, _, a, b in live],
                                    [0.0 if h.scale_max == float("inf") else float(h.scale_max) for h in heads],
                                    [getattr(self, f"{key}_w") for key, _, _, _ in live], row0, b, grad_scale)
        loss = ops.InfoNCEMultiFn.apply(meta, *xs, *scales)
        for k, (key, _, _, _) in enumerate(live):
            self._total_loss[key] += meta.losses[k]
        return loss


def _need_image_features(head, x1):
    if x1 is None:
        raise VipantError(f"{head}: the Barlow heads need image features (x1); with dummy images (the AT script, "
                          "running.imagine / frame_emb) there are none -- model/loss=barlow and barlow_ce are VA-only")


@LOSS_HEADS_REGISTRY.register()
class BarlowLossHead(LossHead):
    """Barlow Twins objective (cvap/module/decoder/loss_head.py:287-328): a projector of bias-free Linears with BatchNorm1d + ReLU
    between them, an affine-free BatchNorm1d, and sum_i (c_ii - 1)^2 + lambd_off sum_{i != j} c_ij^2 of the cross-correlation
    c = bn(z1)^T bn(z2) / B.  Modules and names are the reference's (the state dict loads strictly); the arithmetic of the
    training forward and backward is ops.BarlowFn (HIP batch norm, loss kernel, the library's contractions).  Eval mode caches
    features for the retrieval report (LossHead.infer), as the reference does."""

    def __init__(self, cfg, **kwargs):
        super().__init__()
        self.normalized = False
        sizes = [int(cfg.embed_dim)] + [int(w) for w in cfg.layers]
        if len(sizes) < 2:
            raise VipantError("BarlowLossHead: `layers` needs at least one width (the projector's output)")
        for name, w in [("embed_dim", sizes[0])] + [(f"layers[{i}]", v) for i, v in enumerate(sizes[1:])]:
            if w <= 0 or w % 64:
                raise VipantError(f"BarlowLossHead: {name} = {w} is not a positive multiple of 64 (the projector's contractions "
                                  "need K % 64 == 0)")
        if kwargs.get("negatives", "global") != "global":
            raise VipantError(f"BarlowLossHead: negatives={kwargs.get('negatives')!r} is not built; the Barlow heads use global "
                              "negatives (every replica scores the all-gathered batch)")
        layers = []
        for i in range(len(sizes) - 2):
            layers.extend([nn.Linear(sizes[i], sizes[i + 1], bias=False), nn.BatchNorm1d(sizes[i + 1]), nn.ReLU(inplace=True)])
        layers.append(nn.Linear(sizes[-2], sizes[-1], bias=False))
        self.linear = nn.Sequential(*layers)
        self.bn = nn.BatchNorm1d(sizes[-1], affine=False)
        if any(m.momentum is None for m in self.modules() if isinstance(m, nn.BatchNorm1d)):
            raise VipantError("BarlowLossHead: BatchNorm1d(momentum=None) is not supported")
        self.lambd_off = float(cfg.lambd_off)
        self.reduce = True
        self.parts = None            # fp32 [3] device tensor of the last training forward: loss, on-diagonal, off-diagonal

    def _projector(self):
        mods = list(self.linear)
        lins = [m for m in mods if isinstance(m, nn.Linear)]
        bns = [m for m in mods if isinstance(m, nn.BatchNorm1d)]
        params = []
        for lin, bn in zip(lins[:-1], bns):
            params += [lin.weight, bn.weight, bn.bias]
        params.append(lins[-1].weight)
        return bns, params

    def forward(self, x1, x2, *args, **kwargs):
        if not self.training:
            if not dist.is_initialized() or dist.get_rank() == 0:
                return self.infer(x1, x2, *args, **kwargs)
            return None
        _need_image_features(type(self).__name__, x1)
        b = x1.shape[0]
        row0 = 0
        want_dx1 = x1.requires_grad
        if parallel.active():
            x1, x2 = parallel.all_gather_features(x1, x2)
            row0 = parallel.rank() * b
        bns, params = self._projector()
        meta = ops.BarlowMeta(bns, self.bn, self.lambd_off, row0, b, want_dx1=want_dx1)
        loss = ops.BarlowFn.apply(x1.contiguous(), x2.contiguous(), meta, *params)
        self.parts = meta.parts
        return loss


@LOSS_HEADS_REGISTRY.register()
class BarlowCELossHead(LossHead):
    """InfoNCE + lambd_barlow x Barlow Twins (cvap/module/decoder/loss_head.py:601-622); sub-heads `loss_ce` and `loss_barlow`.
    Eval mode and the report are the InfoNCE head's."""

    CE_DEFAULTS = {"layers": [], "scaling": True, "scale_max": None}     # configs/model/loss/ce.yaml

    def __init__(self, cfg, **kwargs):
        super().__init__()
        self.normalized = False
        ce_cfg = copy.deepcopy(cfg.ce)
        filled = [k for k in self.CE_DEFAULTS if k not in ce_cfg]
        for k in filled:
            ce_cfg[k] = copy.deepcopy(self.CE_DEFAULTS[k])
        if filled and parallel.rank() == 0:
            # barlow_ce.yaml's `ce` group names the head only; CELossHead reads cfg.scaling (a KeyError under Hydra's struct mode)
            logging.getLogger(__name__).warning("BarlowCELossHead: `ce` sub-config has no %s; filled from model/loss=ce (%s)",
                                                ", ".join(filled), ", ".join(f"{k}={ce_cfg[k]}" for k in filled))
        self.loss_ce = build_loss_head(ce_cfg, **kwargs)
        self.loss_barlow = build_loss_head(cfg.barlow, **kwargs)
        self.lambd_barlow = float(cfg.lambd_barlow)
        self.reduce = True

    def report(self, gold_file=None):
        return self.loss_ce.report(gold_file=gold_file)

    def forward(self, x1, x2, *args, **kwargs):
        if not self.training:
            if not dist.is_initialized() or dist.get_rank() == 0:
                return self.loss_ce.infer(x1, x2, *args, **kwargs)
            return None
        _need_image_features(type(self).__name__, x1)
        loss_ce = self.loss_ce(x1, x2, *args, **kwargs)
        loss_barlow = self.loss_barlow(x1, x2, *args, **kwargs)
        return loss_ce + self.lambd_barlow * loss_barlow


def _classifier_widths(who, sizes):
    """Every width of a classification head feeds a LayerNorm and is the K of a contraction: a positive multiple of 64 for
    vipant_gemm_nt, and a multiple of 256 up to 1024 for the library's LayerNorm kernels."""
    for name, w in [("embed_dim", sizes[0])] + [(f"layers[{i}]", v) for i, v in enumerate(sizes[1:])]:
        if w <= 0 or w % 64:
            raise VipantError(f"{who}: {name} = {w} is not a positive multiple of 64 (the head's contractions need K % 64 == 0)")
        if w % 256 or w > 1024:
            raise VipantError(f"{who}: {name} = {w} is not a multiple of 256 up to 1024 (the widths the LayerNorm kernels take)")


class _ClassifierHead(LossHead):
    """What ClassificationHead and BCELossHead share: `linear` = [LayerNorm, Linear] pairs under the reference's names, the
    training forward through ops.ClassifierFn, the eval forward on rank 0 only."""

    kind = "ce"
    soft_targets = False      # BCELossHead: floating-point targets are fractions (mixup), not multi-hot marks

    def _build_linear(self, sizes, last_bias=True):
        from .val import LayerNorm
        _classifier_widths(type(self).__name__, sizes[:-1])
        if int(sizes[-1]) < 1:
            raise VipantError(f"{type(self).__name__}: output_dim = {sizes[-1]} classes")
        layers = []
        for i in range(len(sizes) - 1):
            layers.extend([LayerNorm(sizes[i]), nn.Linear(sizes[i], sizes[i + 1], bias=(last_bias if i == len(sizes) - 2 else True))])
        self.linear = nn.Sequential(*layers)
        self.nclass = int(sizes[-1])

    def _params(self):
        mods = list(self.linear)
        out = []
        for ln, lin in zip(mods[0::2], mods[1::2]):
            out += [ln.weight, ln.bias, lin.weight, lin.bias]
        return out

    def _scale(self, device):
        if isinstance(self.logit_scale, nn.Parameter):
            return self.logit_scale
        return self.logit_scale.to(device) if self.scaling else None

    def _target(self, x2, device):
        if self.kind == "ce":
            return torch.as_tensor(x2, device=device).long().contiguous()
        x2 = torch.as_tensor(x2, device=device)
        if self.soft_targets and x2.is_floating_point():
            return x2.float().contiguous()                                                      # mixup's fractional labels
        return (x2 if x2.dtype == torch.uint8 else (x2 != 0).to(torch.uint8)).contiguous()      # multi-hot: binary targets

    def _run(self, x1, x2, **meta_kwargs):
        params = self._params()
        ls = self._scale(x1.device)
        if not torch.is_grad_enabled():
            params = [None if p is None else p.detach() for p in params]     # nothing will be differentiated: forward-only path
            ls = None if ls is None else ls.detach()
        grad_scale = 1.0 / parallel.world_size() if (parallel.active() and self.training) else 1.0
        target = self._target(x2, x1.device)
        kind = "bce_soft" if (self.kind == "bce" and target.dtype == torch.float32) else self.kind
        meta = ops.ClassifierMeta(kind, self.nclass, grad_scale, **meta_kwargs)
        loss = ops.ClassifierFn.apply(x1.float(), target, ls, meta, *params)
        return loss, meta

    def forward(self, x1, x2, *args, **kwargs):
        """x1: features fp32 [b, E]; x2: labels int [b] (ClassificationHead) or multi-hot targets [b, C] (BCELossHead).  Under
        replicas a rank scores its own rows -- the loss is a mean of per-sample terms, no gather is needed -- and every gradient
        leaves the kernel scaled by 1 / world: the replicas SUM-reduce the head's parameter gradients with the tower's."""
        if not self.training:
            if not dist.is_initialized() or dist.get_rank() == 0:
                return self.infer(x1, x2, *args, **kwargs)
            return None
        return self._run(x1, x2)[0]


@LOSS_HEADS_REGISTRY.register()
class ClassificationHead(_ClassifierHead):
    """Soft-max classifier on audio features (cvap/module/decoder/loss_head.py:330-419): LayerNorm + Linear under `linear.0` /
    `linear.1`, a learnable temperature, nn.CrossEntropyLoss.  Training: ops.ClassifierFn.  Eval: `infer` caches features,
    arg-max predictions (the loss kernel's `pred`) and labels; `report` is the supervised precision or, with `text`, the
    zero-shot one (zero_shot_report)."""

    kind = "ce"

    def __init__(self, cfg, **kwargs):
        super().__init__()
        self.normalized = False
        if "output_dim" not in kwargs:
            raise VipantError("ClassificationHead: `the label number` is not found in `kwargs` (output_dim)")
        self._build_linear([int(cfg.embed_dim), int(kwargs["output_dim"])])
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.scaling = True
        self.reduce = False

    def copy_state_dict(self, state_dict):
        new_dict = self.state_dict()
        new_dict.update({k: v for k, v in state_dict.items() if k in new_dict})
        self.load_state_dict(new_dict)

    def infer(self, x1, x2, *args, **kwargs):
        if not hasattr(self, "audios") or not hasattr(self, "x1s") or not hasattr(self, "x2s") or not hasattr(self, "ids"):
            self.audios, self.x1s, self.x2s, self.ids = [], [], [], []
        with torch.no_grad():
            _, meta = self._run(x1.detach(), x2, want_pred=True)
        self.audios.append(x1.detach().float())
        self.x1s.append(meta.pred.long())
        self.x2s.append(torch.as_tensor(x2, device=x1.device).long())
        names = kwargs.get("names", None)
        if names is not None:
            self.ids.extend(names)
        return None

    def report(self, gold_file=None, **kwargs):
        x1s, x2s = torch.cat(self.x1s), torch.cat(self.x2s)
        nsample = len(x1s)
        text = kwargs.get("text", None)
        if text is not None:
            out = zero_shot_report(torch.cat(self.audios), x2s, text, kwargs.get("label_map", None))
        else:
            precision = (x1s == x2s).sum() / nsample * 100.       # float32 tensor, as in the reference
            out = f"A->T: p1 = {precision:2.2f} @ {nsample}"
        del self.audios, self.x1s, self.x2s, self.ids
        return out


@LOSS_HEADS_REGISTRY.register()
class BCELossHead(_ClassifierHead):
    """Multi-label tagging head (cvap/module/decoder/loss_more.py:29-143): `cfg.layers` hidden widths give LayerNorm / Linear
    pairs `linear.{2i}` / `linear.{2i+1}`, the last Linear has `bias=cfg.bias`; nn.BCEWithLogitsLoss on exp(logit_scale) x logits
    (`scaling: False`: a plain tensor of 0, scale 1).  Eval: `infer` returns the loss and caches the sigmoid scores; `report`
    is the reference's string with its scikit-learn quantities restated in numpy (vipant_amd/util/metrics.py).
    `soft_targets` (`cfg.soft_targets`, default False; ASMonitor sets it when `running.mixup_rate > 0`): floating-point targets
    go to the soft-target kernel as fractions instead of being binarised; integer targets take the binary kernel either way.
    The gold labels `infer` caches for `report` stay binary (evaluation data is never mixed)."""

    kind = "bce"

    def __init__(self, cfg, **kwargs):
        super().__init__()
        self.normalized = False
        if "output_dim" not in kwargs:
            raise VipantError("BCELossHead: `the label number` is not found in `kwargs` (output_dim)")
        embed_dim = cfg.embed_dim or cfg.width
        self._build_linear([int(embed_dim)] + [int(w) for w in cfg.layers] + [int(kwargs["output_dim"])], last_bias=bool(cfg.bias))
        self.scaling = bool(cfg.scaling)
        self.logit_scale = (nn.Parameter(torch.ones([]) * np.log(1 / 0.07)) if cfg.scaling
                            else torch.ones([], requires_grad=False) * np.log(1 / 1))
        self.reduce = False
        self.soft_targets = bool(getattr(cfg, "soft_targets", False))      # = cfg.get("soft_targets", False), for namespace configs too

    def copy_state_dict(self, state_dict):
        key = "logit_scale"
        new_dict = self.state_dict()
        new_dict.update({key: state_dict[key]})
        self.load_state_dict(new_dict)

    def infer(self, x1, x2, *args, **kwargs):
        if not hasattr(self, "audios") or not hasattr(self, "x1s") or not hasattr(self, "x2s") or not hasattr(self, "ids"):
            self.audios, self.x1s, self.x2s, self.ids = [], [], [], []
        with torch.no_grad():
            loss, meta = self._run(x1.detach(), x2, want_prob=True)
        self.audios.append(x1.detach().float())
        self.x1s.append(meta.prob)
        x2 = torch.as_tensor(x2, device=x1.device)
        self.x2s.append((x2 != 0).to(x2.dtype) if (self.soft_targets and x2.is_floating_point()) else x2)
        names = kwargs.get("names", None)
        if names is not None:
            self.ids.extend(names)
        return loss

    def zero_shot(self, text, gold_file):
        audios = ops.l2_normalize(torch.cat(self.audios).contiguous())
        text = ops.l2_normalize(text.detach().float().contiguous())
        nclass = text.shape[0]
        if nclass % 4:      # the similarity contraction needs a multiple of 4 prompts (AudioSet has 527): zero rows, their columns dropped
            text = torch.cat([text, text.new_zeros((4 - nclass % 4, text.shape[1]))]).contiguous()
        x1s = torch.empty((audios.shape[0], text.shape[0]), dtype=torch.float32, device=audios.device)
        a16, t16 = ops.cast_bf16(audios)[0], ops.cast_bf16(text)[0]
        ops.gemm_nt(a16, t16, x1s, epi=ops.EPI_F32)
        return self.report(gold_file=gold_file, text=None, x1s=x1s[:, :nclass].contiguous().cpu().numpy())

    def report(self, gold_file=None, x1s=None, x2s=None, **kwargs):
        from ..util.metrics import multilabel_report
        text = kwargs.get("text", None)
        if text is not None:
            return self.zero_shot(text, gold_file)
        x1s = torch.cat(self.x1s).cpu().numpy() if x1s is None else x1s
        x2s = torch.cat(self.x2s).cpu().numpy() if x2s is None else x2s
        del self.audios, self.x1s, self.x2s, self.ids
        return multilabel_report(x2s, x1s)


class DummyLossHead(nn.Module):
    def __init__(self, cfg, **kwargs):
        super().__init__()

    def forward(self, *args, **kwargs):
        return None
