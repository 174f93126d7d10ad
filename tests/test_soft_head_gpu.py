"""`+model/loss=ce_soft`, `ce_val_soft` through the public interface against float64 autograd through normalise + the restated loss of
tests/test_soft_nce_gpu.py; a given teacher takes no gradient; the un-listed pair; two replicas over gloo against one process."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import vipant_amd.module as M
from test_label_head_gpu import B, DEV, inputs
from test_replicas_gpu import _free_port
from test_sigmoid_loss_gpu import close
from test_soft_nce_gpu import reference, scalars_ok
from vipant_amd._ffi import VipantError
from vipant_amd.config import compose, to_config

pytestmark = pytest.mark.gpu


def build_head(name, negatives="global", **over):
    return M.build_loss_head(to_config(dict(compose([f"+model/loss={name}"]).model.loss, **over)), negatives=negatives).to(DEV)


def step(head, xs, **kw):       # [loss, d leaves, d logit_scale(s)]
    leaves = [x.clone().requires_grad_() for x in xs]
    loss = head.train()(*leaves, normalized=False, **kw)
    loss.backward()
    return [loss.detach()] + [v.grad for v in leaves] + [p.grad for p in head.parameters()]


@pytest.mark.parametrize("teacher,w", [("x2", (-1.0, 1.0)), ("x1", (0.0, 1.0)), ("given", (0.5, 4.0))])
def test_head_against_fp64_autograd(teacher, w):
    xs, head = inputs(3), build_head("ce_soft", teacher=teacher, w_floor=w[0], w_power=w[1])
    given = xs[2][:, :128].clone().requires_grad_()         # Et != E
    if teacher == "given":
        with pytest.raises(VipantError, match="teacher"):
            head.train()(xs[0], xs[1], normalized=False)
    got = step(head, xs[:2], **({"teacher": given} if teacher == "given" else {}))
    assert given.grad is None
    leaves = [x.double().requires_grad_() for x in xs[:2]]
    n = [torch.nn.functional.normalize(x, dim=-1) for x in leaves]
    x1, x2 = (v.detach().float() for v in n)
    t = {"x1": x1, "x2": x2, "given": torch.nn.functional.normalize(given.detach(), dim=-1)}[teacher]
    ls = float(head.logit_scale.detach())
    ref, emu, up, down = (reference(x1, x2, t, ls, wf=w[0], wp=w[1], emulate=e, dc=d)
                          for e, d in ((False, 0.0), (True, 0.0), (False, 2.0 ** -18), (False, -2.0 ** -18)))
    bad = scalars_ok({"loss": got[0], "dls": got[3]}, ref, [ref, up, down])
    want, bound = (torch.autograd.grad(n, leaves, [r["dx1"], r["dx2"]], retain_graph=True) for r in (ref, emu))
    bad += [k for k in (0, 1) if not close(f"dx{k + 1}", got[1 + k], want[k], bound[k])]
    assert not bad, bad


def test_unlisted_pair_is_ce_val_bit_for_bit():
    xs = inputs(3)
    head, plain = build_head("ce_val_soft", soft_positives={"al": "x2"}), build_head("ce_val")
    got, ref = step(head, xs), step(plain, xs)
    assert type(head.loss_head_va) is M.CELossHead and type(head.loss_head_al) is M.SoftCELossHead
    assert torch.equal(head._total_loss["va"], plain._total_loss["va"]) and torch.equal(got[1], ref[1])     # the image: read by va only
    assert not torch.equal(head._total_loss["al"], plain._total_loss["al"])


def _run(rank, world, port, out):
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        xs = inputs(3)
        sl = slice(rank * (B // world), (rank + 1) * (B // world))
        res = step(build_head("ce_soft", teacher="given"), [x[sl] for x in xs[:2]], teacher=xs[2][sl])
        torch.save([v.cpu() for v in res], f"{out}.{rank}")
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_replicas_match_single_process_soft(tmp_path):
    mp.spawn(_run, args=(1, 0, str(tmp_path / "one")), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), str(tmp_path / "two")), nprocs=2, join=True)
    a = torch.load(tmp_path / "one.0")
    for r in (0, 1):
        t = torch.load(tmp_path / f"two.{r}")
        assert abs(float(a[0] - t[0])) <= 1e-5 * max(1.0, abs(float(a[0]))), (r, a[0], t[0])
        for k in (1, 2, 3):         # dx1, dx2: this rank's rows; dlogit_scale: complete on every rank
            want = a[k][r * B // 2:(r + 1) * B // 2] if k < 3 else a[k]
            assert float((want - t[k]).abs().max()) <= 1e-6 + 2e-4 * float(want.abs().max()), (r, k)
