"""`optimizer.optimizer=[LAMB, {...}]` in the trainer: the configuration of tests/test_adam_trainer_gpu.py, one step, run twice from the
same seed -- with the default (the fused launch group) and with `+optimizer.fused_step=False` (the class's plain torch step).  The
forward runs before any update, so the losses are the same bits; the gradients are the same, so only the update differs, and it is
held to the bound of tests/test_lamb_gpu.py: the float64 rule (tests/lamb_ref.py) on the run's own parameters and gradients is the
reference, the plain run's distance from it the yardstick, the fused run may be 2 x as far off plus one ulp."""
import numpy as np
import pytest
import torch

import lamb_ref as R
from test_adam_trainer_gpu import _one_step
from test_lamb_gpu import _maxabs, _tolerances

pytestmark = pytest.mark.gpu

LAMB_CFG = ["optimizer.optimizer=[LAMB, {lr: 0.001, weight_decay: 0.01, max_grad_norm: 1.0}]"]


def test_one_trainer_step_fused_against_plain():
    import vipant_amd.module as M
    fused, p0, p_fused, g_fused = _one_step(LAMB_CFG)
    plain, q0, p_plain, g_plain = _one_step(LAMB_CFG + ["+optimizer.fused_step=False"])
    assert type(fused.optimizer) is M.LAMB and fused.optimizer.fused and type(plain.optimizer) is M.LAMB and not plain.optimizer.fused
    assert "_vipant_fused" in vars(fused.optimizer) and "_vipant_fused" not in vars(plain.optimizer)
    assert torch.equal(fused.total_loss, plain.total_loss) and bool(torch.isfinite(fused.total_loss))       # forward before any update
    assert p0.keys() == q0.keys() and all(torch.equal(p0[k], q0[k]) for k in p0)
    assert g_fused.keys() == g_plain.keys() and g_fused and all(torch.equal(g_fused[k], g_plain[k]) for k in g_fused)
    names, tensors = [], []
    for group in fused.optimizer.param_groups:
        ids = {id(p) for p in group["params"]}
        for k, p in fused.model.named_parameters():
            if id(p) in ids and k in g_fused:
                adapt = p.ndim > 1
                names.append(k)
                tensors.append(dict(p=p0[k].cpu().numpy().ravel(), g=g_fused[k].cpu().numpy().ravel(), m=0.0, v=0.0, lr=group["lr"], eps=group["eps"],
                                    wd=group["weight_decay"] if adapt else 0.0, adapt=adapt, step=1))
    assert sorted(names) == sorted(g_fused)
    G, c, ref = R.lamb_step_f64(tensors, beta1=0.9, beta2=0.999, max_grad_norm=1.0)
    assert abs(float(fused.optimizer._vipant_fused[1].grad_norm) - G) <= R.G_REL * G
    want = [r[0] for r in ref]
    got, yard = ([x[k].double().cpu().numpy().ravel() for k in names] for x in (p_fused, p_plain))
    ratios = [_maxabs(a - b) / t for a, b, t in zip(got, want, _tolerances(yard, want))]
    print(f"LAMB-TRAINER: {len(names)} tensors, G = {G:.4f}, c = {c:.4f}, max |fused - f64| / tolerance = {max(ratios):.3f}")
    assert max(ratios) <= 1.0, names[int(np.argmax(ratios))]
    assert all(not torch.equal(p_fused[k], p0[k]) for k in names)
