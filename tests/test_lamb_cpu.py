"""LAMB without a GPU: the class's plain torch step is the float64 rule of tests/lamb_ref.py (the oracle of tests/test_lamb_gpu.py),
`Monitor.build_optimizer` resolves the name, and the C entry points report bad arguments and launch nothing."""
import types

import numpy as np
import pytest
import torch

import lamb_ref as R


@pytest.mark.parametrize("max_grad_norm", [0.0, 0.05, 1e3])          # off, binding, not binding
@pytest.mark.parametrize("exclude", [True, False])
def test_plain_step_is_the_float64_rule(exclude, max_grad_norm):
    from vipant_amd.module import LAMB
    rng = np.random.default_rng(11)
    shapes = [(6, 5), (4, 3), (7,), (3, 2), (5,)]
    p0 = [rng.standard_normal(s) for s in shapes]
    p0[1][:] = 0.0                                                      # |p| = 0: phi = 1
    params = [torch.nn.Parameter(torch.tensor(x)) for x in p0]           # float64 parameters: float64 moments
    groups = [{"params": params[:3]}, {"params": params[3:], "weight_decay": 0.0, "lr": 5e-3, "eps": 1e-5}]
    opt = LAMB(groups, lr=2e-3, betas=(0.9, 0.99), weight_decay=0.02, max_grad_norm=max_grad_norm, exclude_bias_and_norm=exclude, fused=False)
    cur = [dict(p=x.copy(), m=np.zeros_like(x), v=np.zeros_like(x)) for x in p0]
    for step in (1, 2, 3):
        grads = [rng.standard_normal(s) * 0.1 for s in shapes]
        grads[3][:] = 0.0                                               # zero gradient, wd = 0: |u| = 0, phi = 1
        for p, g in zip(params, grads):
            p.grad = torch.tensor(g)
        opt.step()
        for i, (t, g) in enumerate(zip(cur, grads)):
            group = opt.param_groups[0 if i < 3 else 1]
            adapt = not (exclude and len(shapes[i]) < 2)
            t.update(g=g, lr=group["lr"], eps=group["eps"], wd=group["weight_decay"] if adapt else 0.0, adapt=adapt, step=step)
        G, c, new = R.lamb_step_f64(cur, beta1=0.9, beta2=0.99, max_grad_norm=max_grad_norm)
        assert (c < 1.0) == (max_grad_norm == 0.05)
        for t, (p1, m1, v1), p in zip(cur, new, params):
            t.update(p=p1, m=m1, v=v1)
            for want, got in ((p1, p), (m1, opt.state[p]["exp_avg"]), (v1, opt.state[p]["exp_avg_sq"])):
                assert np.max(np.abs(want - got.detach().numpy())) <= 1e-13 * max(1.0, np.max(np.abs(want)))
    assert not np.array_equal(cur[1]["p"], p0[1]) and np.array_equal(cur[3]["p"], p0[3])
    assert all(float(opt.state[p]["step"]) == 3.0 and opt.state[p]["step"].is_cpu for p in params)


def test_build_optimizer_resolves_lamb():
    import vipant_amd.module as M
    import cvap.module
    from vipant_amd.config import compose
    from vipant_amd.monitor import Monitor
    assert cvap.module.LAMB is M.LAMB
    base = ("+running=bimodal worker=CVALP +model/image=vit_val +model/audio=vit_val +model/text=dummy +model/loss=ce "
            "+optimizer=standard +running/audio=default optimizer.use_lars=False").split()
    for extra, fused in (([], True), (["+optimizer.fused_step=False"], False)):
        model = torch.nn.Linear(4, 3).train()
        model.audio_head = None
        mon = types.SimpleNamespace(model=model, echo=lambda *_: None,
                                    cfg=compose(base + ["optimizer.optimizer=[LAMB, {lr: 0.001, max_grad_norm: 1.0}]"] + extra))
        Monitor.build_optimizer(mon, dict(model.named_parameters()))
        assert type(mon.optimizer) is M.LAMB and mon.optimizer.fused is fused
        assert [g["max_grad_norm"] for g in mon.optimizer.param_groups] == [1.0, 1.0] and mon.optimizer.param_groups[0]["lr"] == 1e-3
        assert [[p.ndim for p in g["params"]] for g in mon.optimizer.param_groups] == [[2], [1]]
        assert isinstance(mon.scheduler, torch.optim.lr_scheduler.MultiStepLR) and "initial_lr" in mon.optimizer.param_groups[0]
    from vipant_amd.errors import VipantError
    with pytest.raises(VipantError, match="one non-negative value per optimizer"):
        M.LAMB([{"params": [torch.nn.Parameter(torch.zeros(2))]}, {"params": [torch.nn.Parameter(torch.zeros(2))], "max_grad_norm": 1.0}])


def test_bad_arguments_are_reported_not_executed():
    from vipant_amd import _ffi
    ok, good = [16] * 7, (3, 1, 8192, 0.9, 0.999, 1.0, 16, 1 << 20, None)          # (never dereferenced: every call below is refused)
    need = _ffi.query("vipant_lamb_workspace_bytes", 3, 5)
    assert need == 4 * (4 + 4 + 3 * 8) and _ffi.query("vipant_grad_norm_workspace_bytes", 5) == 4 * (4 + 8)
    cases = [("null table", [None if i == k else 16 for i in range(7)], good) for k in range(7)]
    cases += [("multiple of 1024", ok, (3, 1, chunk) + good[3:]) for chunk in (0, 1000, 8192 + 4, 1 << 21)]
    cases += [("bad tensor count 0", ok, (0,) + good[1:]), ("betas", ok, good[:4] + (1.0,) + good[5:]),
              ("max_grad_norm must be >= 0", ok, good[:5] + (-1.0,) + good[6:])]
    cases += [("code -5: lamb_step: workspace", ok, (3, 5) + good[2:6] + (ws, nbytes, None))
              for ws, nbytes in ((16, need - 1), (None, need), (20, need))]             # short, NULL, misaligned
    for match, tables, rest in cases:
        with pytest.raises(_ffi.VipantError, match=match):
            _ffi.call("vipant_lamb_step", *tables, *rest)
    for match, args in (("grad_norm: null table", (16, 16, 16, 3, 5, 8192, None, 16, 1 << 20, None)),
                        ("grad_norm: bad chunk count", (16, 16, 16, 3, 0, 8192, 16, 16, 1 << 20, None)),
                        ("grad_norm: workspace", (16, 16, 16, 3, 5, 8192, 16, 16, 4 * (4 + 8) - 1, None))):
        with pytest.raises(_ffi.VipantError, match=match):
            _ffi.call("vipant_grad_norm", *args)
