"""`+model/loss=ce_label`, `ce_val_label` through the public interface against float64 autograd through normalise + the restated loss of
tests/test_label_nce_gpu.py; identity positives; the un-listed pair; two replicas over gloo against one process; two trainer steps."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import vipant_amd.module as M
from test_label_nce_gpu import groups_of, reference
from test_sigmoid_loss_gpu import close
from vipant_amd.config import compose

pytestmark = pytest.mark.gpu
DEV, B, E = "cuda:0", 48, 512


build_head = lambda name, **kwargs: M.build_loss_head(compose([f"+model/loss={name}"]).model.loss, **kwargs).to(DEV)  # noqa: E731


def inputs(n):
    g = torch.Generator().manual_seed(n)
    base = torch.randn(B, E, generator=g)
    return [(3.0 * (base + 0.7 * torch.randn(B, E, generator=g))).to(DEV) for _ in range(n)]       # un-normalised: the head normalises


def step(head, xs, ids):
    leaves = [x.clone().requires_grad_() for x in xs]
    loss = head.train()(*leaves, normalized=False, groups=ids)
    loss.backward()
    return [loss.detach()] + [v.grad for v in leaves] + [p.grad for p in head.parameters()]


def restated(xs, scales, ids):      # [loss, d leaves, d scales] in float64; the bf16 emulation pushed through the normalisation
    leaves = [x.double().requires_grad_() for x in xs]
    scales = [torch.tensor(float(v), dtype=torch.float64, device=DEV, requires_grad=True) for v in scales]
    n = [torch.nn.functional.normalize(x, dim=-1) for x in leaves]
    pairs = [(0, 1, ids)] if len(xs) == 2 else [(0, 1, None), (1, 2, ids)]          # ce_label | ce_val_label: va plain, al labelled
    loss = sum(reference(n[a], n[b], g, s)["loss"] for (a, b, g), s in zip(pairs, scales))
    want = torch.autograd.grad(loss, leaves + scales, retain_graph=True)
    cot = [torch.zeros_like(x) for x in leaves]
    for (a, b, g), s in zip(pairs, scales):
        emu = reference(n[a].detach(), n[b].detach(), g, float(s.detach()), emulate=True)
        cot[a], cot[b] = cot[a] + emu["dx1"], cot[b] + emu["dx2"]
    return [loss.detach(), *want], [None, *torch.autograd.grad(n, leaves, cot), *[None] * len(scales)]


@pytest.mark.parametrize("name,n", [("ce_label", 2), ("ce_val_label", 3)])
def test_head_against_fp64_autograd(name, n):
    xs, ids, head = inputs(n), groups_of("mod3", B).to(DEV), build_head(name)
    got = step(head, xs, ids)
    want, emu = restated(xs, [p.detach() for p in head.parameters()], ids)
    bad = [i for i in range(len(got)) if not close(f"{name}[{i}]", got[i], want[i], emu[i])]
    assert not bad, bad
    plain = build_head("ce_val" if n == 3 else "ce")
    ref = step(plain, xs, None)
    if n == 3:          # the un-listed va pair is ce_val's, bit for bit: its loss term and the gradient of the operand only it reads
        assert torch.equal(head._total_loss["va"], plain._total_loss["va"]) and torch.equal(got[1], ref[1])
    else:               # identity positives: CELossHead's loss
        assert abs(float(step(head, xs, None)[0] - ref[0])) <= 5e-5 * abs(float(ref[0]))


def _run(rank, world, port, out):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        xs, ids = inputs(2), groups_of("mod3", B)
        sl = slice(rank * (B // world), (rank + 1) * (B // world))
        res = step(build_head("ce_label", negatives="global"), [x[sl] for x in xs], ids[sl])
        torch.save([v.cpu() for v in res], f"{out}.{rank}")
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_replicas_match_single_process_label(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_run, args=(1, 0, str(tmp_path / "one")), nprocs=1, join=True)
    mp.spawn(_run, args=(2, port, str(tmp_path / "two")), nprocs=2, join=True)
    a = torch.load(tmp_path / "one.0")
    for r in (0, 1):
        t = torch.load(tmp_path / f"two.{r}")
        assert abs(float(a[0] - t[0])) <= 1e-5 * max(1.0, abs(float(a[0]))), (r, a[0], t[0])
        for k in (1, 2, 3):         # dx1, dx2: this rank's rows; dlogit_scale: complete on every rank
            want = a[k][r * B // 2:(r + 1) * B // 2] if k < 3 else a[k]
            assert float((want - t[k]).abs().max()) <= 1e-6 + 2e-4 * float(want.abs().max()), (r, k)


def test_trainer_hands_real_label_ids_to_the_head(tmp_path):        # toy AudioSet directory: the labels; synthetic: None, said once
    import audioset_text_fixture as TF
    from test_audioset_text_trainer_gpu import KEY, TRI, _losses, _monitor
    ov = TRI.replace("+model/loss=ce_val", "+model/loss=ce_val_label") + KEY + " eval=False"
    TF.make_dir(str(tmp_path), embed_dim=E, num_mel_bins=64)
    for root in (str(tmp_path), None):
        mon, lines = _monitor(ov, root)
        head, seen = mon.model.loss_head.loss_head_al, []
        head.register_forward_pre_hook(lambda m, a, k: seen.append(k.get("groups")) if m.training else None, with_kwargs=True)
        mon.learn()
        steps = _losses(lines)
        assert [s[0] for s in steps] == ["1", "2"] and all(0.0 < float(s[1]) < 20.0 for s in steps) and mon.label_groups == (root is not None), lines
        assert sum("identity positives" in m for m in lines) == (root is None), lines
        assert len(seen) == 2 and all((g is None) if root is None else (g.dtype == torch.int64 and g.shape == (4,) and g.is_cuda) for g in seen)
