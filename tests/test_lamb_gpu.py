"""The fused LAMB step on the MI355X (vipant_lamb_step / vipant_grad_norm, ops.LambState, ops.grad_norm, vipant_amd.module.LAMB)
against the float64 rule of tests/lamb_ref.py.  Yardstick for parameters and moments: the distance of the class's
own plain fp32 torch step, on the same inputs on the device, from the float64 result -- per tensor the largest absolute difference;
every element of the fused result may be 2 x that far off, plus one fp32 ulp of the tensor's largest value.  Tensors below 48 elements
take the largest relative distance of the list instead of their own (the maximum of a handful of rounding errors is no stable measure)."""
import copy
import functools

import numpy as np
import pytest
import torch

import lamb_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
B1, B2, NSTEPS = 0.9, 0.99, 3
MGN = {"off": 0.0, "binding": 1.0, "loose": 1e4}          # G of the list is about 100
# every edge of the chunking (chunk 8192), 1-D (exempt under exclude_bias_and_norm) and 2-D alternating; a 2-D tensor; a view one element
# into its storage; a zero tensor; a tensor with zero gradients and wd = 0
SHAPES = [(1,), (1, 3), (1023,), (1, 1024), (1025,), (1, 8191), (8192,), (1, 8193), (2 * 8192 + 5,), (96, 200), (3, 86), (40, 50), (30, 20)]
MISALIGNED, ZERO_P, ZERO_G = 10, 11, 12


def _maxabs(x):
    return float(np.max(np.abs(x))) if x.size else 0.0


def _tolerances(plain, ref):
    """Per tensor: 2 x the plain step's distance + one ulp of the largest value (module docstring)."""
    rel = [_maxabs(a - b) / _maxabs(b) if _maxabs(b) > 0 else 0.0 for a, b in zip(plain, ref)]
    return [2.0 * (r if b.size >= 48 else max(rel)) * _maxabs(b) + float(np.spacing(np.float32(_maxabs(b)))) for r, b in zip(rel, ref)]


@functools.lru_cache(maxsize=None)
def _problem():
    rng = np.random.default_rng(35)
    n = [int(np.prod(s)) for s in SHAPES]
    offs, cur = [], 8
    for i, k in enumerate(n):
        cur = (cur + 3) // 4 * 4 + (1 if i == MISALIGNED else 0)
        offs.append(cur)
        cur += k + 4                                       # sentinels between any two tensors
    p = [rng.standard_normal(k).astype(np.float32) * (i != ZERO_P) for i, k in enumerate(n)]
    g = [[(rng.standard_normal(k) * 10.0 ** rng.uniform(-2, 0, k)).astype(np.float32) * (i != ZERO_G) for i, k in enumerate(n)]
         for _ in range(NSTEPS)]
    hyper = [dict(lr=1e-3 * (1 + i % 3), eps=1e-6, adapt=len(s) > 1, wd=0.01 if len(s) > 1 and i != ZERO_G else 0.0) for i, s in enumerate(SHAPES)]
    return n, offs, cur + 8, p, g, hyper


@functools.lru_cache(maxsize=None)
def _reference(mgn):
    """Per step: the float64 result (G, c, [(p, m, v)]) and the plain fp32 device step's result ([p], [m], [v]) from the same inputs."""
    from vipant_amd.module import LAMB
    n, _, _, p, g, hyper = _problem()
    cur = [dict(h, p=x, m=np.zeros_like(x), v=np.zeros_like(x)) for h, x in zip(hyper, p)]
    dev = [(torch.tensor(x, device=DEV), dict(step=torch.tensor(0.0), exp_avg=torch.zeros(len(x), device=DEV), exp_avg_sq=torch.zeros(len(x), device=DEV)))
           for x in p]
    out = []
    for s in range(NSTEPS):
        for t, gs in zip(cur, g[s]):
            t.update(g=gs, step=s + 1)
        G, c, new = R.lamb_step_f64(cur, beta1=B1, beta2=B2, max_grad_norm=mgn)
        for t, (p1, m1, v1) in zip(cur, new):
            t.update(p=p1, m=m1, v=v1)
        LAMB._plain_step([(w, torch.tensor(gs, device=DEV), st, (h["lr"], h["wd"], h["eps"], B1, B2, h["adapt"]))
                          for (w, st), gs, h in zip(dev, g[s], hyper)], mgn)
        plain = [[x.double().cpu().numpy() for x in xs] for xs in ([w for w, _ in dev], [st["exp_avg"] for _, st in dev], [st["exp_avg_sq"] for _, st in dev])]
        out.append((G, c, [list(q) for q in zip(*new)], plain))
    return out


@functools.lru_cache(maxsize=None)
def _fused(mgn, width, fill):
    """Three fused steps on views of sentinel-filled buffers, the workspace (exactly vipant_lamb_workspace_bytes, between sentinels)
    pre-filled with `fill` -> per step (flat p, m, v, g buffers, G of ops.grad_norm, G and c of the step)."""
    from vipant_amd import ops
    n, offs, total, p, g, hyper = _problem()
    flat = {k: torch.full((total,), -1234.5, device=DEV) for k in "pgmv"}
    views = {k: [flat[k][o:o + c].view(s) for o, c, s in zip(offs, n, SHAPES)] for k in "pgmv"}
    for i, x in enumerate(p):
        views["p"][i].copy_(torch.tensor(x).view(SHAPES[i])); views["m"][i].zero_(); views["v"][i].zero_()
    assert views["p"][MISALIGNED].data_ptr() % 16 == 4 and views["p"][9].data_ptr() % 16 == 0
    nchunks = sum(-(-k // ops.AdamState.chunk_elements()) for k in n)
    need = ops.LambState.workspace_bytes(len(n), nchunks)
    wsbuf = torch.full(((need + 32) // 4,), fill, device=DEV)
    state = ops.LambState(views["p"], views["m"], views["v"], workspace=wsbuf.view(torch.uint8)[16:16 + need])
    out = []
    for s in range(NSTEPS):
        for i, x in enumerate(g[s]):
            views["g"][i].copy_(torch.tensor(x).view(SHAPES[i]))
        before = flat["g"].clone()
        G = ops.grad_norm(views["g"])
        state.step(views["g"], [ops.LambState.record(h["lr"], h["wd"], h["eps"], B1, B2, s + 1, h["adapt"]) for h in hyper], B1, B2, mgn)
        assert torch.equal(flat["g"], before)                                       # gradients are read only
        out.append(({k: flat[k].cpu().numpy() for k in "pmv"}, float(G), float(state.grad_norm), float(state.clip_coef)))
    edges = wsbuf.view(torch.int32).cpu().numpy()
    assert len(set(edges[:4]) | set(edges[-4:])) == 1, "a sentinel beside the workspace was overwritten"
    return out


@pytest.mark.parametrize("width", [4, 16])
@pytest.mark.parametrize("clip", list(MGN))
def test_steps_against_float64(clip, width, monkeypatch):
    monkeypatch.setenv("VIPANT_LAMB_WIDTH", str(width))
    n, offs, total, _, _, _ = _problem()
    inside = np.zeros(total, bool)
    for o, k in zip(offs, n):
        inside[o:o + k] = True
    for s, ((flat, G, G_step, c_step), (G64, c64, ref, plain)) in enumerate(zip(_fused(MGN[clip], width, float("nan")), _reference(MGN[clip]))):
        print(f"LAMB step {s + 1} clip={clip} width={width}: G error / bound {abs(G - G64) / (R.G_REL * G64):.3f}")
        assert abs(G - G64) <= R.G_REL * G64                  # fp32 within a chunk (32 + 8 deep), fp64 across chunks: lamb_ref.py
        if MGN[clip] > 0:
            assert G_step == G and abs(c_step - c64) <= R.C_REL * c64 and (c64 < 1.0) == (clip == "binding")
        for k, want, yard in zip("pmv", ref, plain):
            assert np.all(flat[k][~inside] == np.float32(-1234.5)), f"{k}: a sentinel was overwritten"
            tol = _tolerances(yard, want)
            err = [np.abs(flat[k][o:o + c].astype(np.float64) - w) for o, c, w in zip(offs, n, want)]
            ratio = max(_maxabs(e) / t for e, t in zip(err, tol))
            print(f"LAMB step {s + 1} clip={clip} width={width} {k}: worst |fused - f64| / tolerance {ratio:.3f}")
            assert all(np.all(e <= t) for e, t in zip(err, tol)), (k, s, ratio)
    assert np.any(flat["p"][offs[ZERO_P]:offs[ZERO_P] + n[ZERO_P]] != 0)               # |p| = 0: phi = 1, the tensor still moves


@pytest.mark.parametrize("width", [4, 16])
def test_same_bits_whatever_the_workspace_held(width, monkeypatch):
    monkeypatch.setenv("VIPANT_LAMB_WIDTH", str(width))
    for (a, *ga), (b, *gb) in zip(_fused(1.0, width, float("nan")), _fused(1.0, width, 3e38)):
        assert ga == gb and all(np.array_equal(a[k], b[k]) for k in "pmv")


# ------------------------------------------------------------------------------------------------- through the class
KW = dict(lr=2e-3, betas=(B1, B2), weight_decay=0.01, max_grad_norm=1.0)
CLS_SHAPES = [(33, 5), (64,), (8192 + 9,), (20, 7)]


def _drive(opt, params, steps, sched=None, written=True):
    rng = np.random.default_rng(8)
    grads = [[rng.standard_normal(s).astype(np.float32) for s in CLS_SHAPES] for _ in range(4)]
    for s in steps:
        if s == 1 and written:
            opt.param_groups[0]["lr"] *= 0.3                                        # by hand; MultiStepLR halves after step 3
        for i, p in enumerate(params):
            p.grad = None if (i, s) == (1, 1) else torch.tensor(grads[s][i], dtype=p.dtype, device=p.device)
        opt.step()
        if sched is not None:
            sched.step()


def _make(fused, dtype=torch.float32, device=DEV, source=None):
    from vipant_amd.module import LAMB
    rng = np.random.default_rng(9)
    params = [torch.nn.Parameter(torch.tensor(rng.standard_normal(s), dtype=dtype, device=device)) for s in CLS_SHAPES]
    opt = LAMB(params, fused=fused, **KW)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[3], gamma=0.5)
    if source is not None:                      # a checkpoint, as torch.save / torch.load would hand it over
        for p, q in zip(params, source[0]):
            p.data.copy_(q.data)
        opt.load_state_dict(copy.deepcopy(source[1].state_dict()))
        sched.load_state_dict(source[2].state_dict())
    return params, opt, sched


def test_checkpoints_learning_rates_and_adam_state():
    import vipant_amd.module as M
    runs = {}
    for name, (fused, dtype, device) in dict(f64=(False, torch.float64, "cpu"), plain=(False, torch.float32, DEV), fused=(True, torch.float32, DEV)).items():
        params, opt, sched = runs[name] = _make(fused, dtype, device)
        _drive(opt, params, range(1), sched)
        kept = [x.clone() for x in (params[1].detach(), opt.state[params[1]]["exp_avg"], opt.state[params[1]]["exp_avg_sq"])]
        _drive(opt, params, range(1, 2), sched)
        # no gradient at step 2: value, moments and count are kept
        assert all(torch.equal(a, b) for a, b in zip(kept, (params[1].detach(), opt.state[params[1]]["exp_avg"], opt.state[params[1]]["exp_avg_sq"])))
        assert float(opt.state[params[1]]["step"]) == 1.0 and float(opt.state[params[0]]["step"]) == 2.0
    assert "_vipant_fused" in vars(runs["fused"][1]) and "_vipant_fused" not in vars(runs["plain"][1])
    # the checkpoint crosses over mid-trajectory, both ways
    runs["fused->plain"], runs["plain->fused"] = _make(False, source=runs["fused"]), _make(True, source=runs["plain"])
    for name, (params, opt, sched) in runs.items():
        _drive(opt, params, range(2, 4), sched)
        assert abs(opt.param_groups[0]["lr"] - KW["lr"] * 0.3 * 0.5) < 1e-15, name
    snap = {name: [p.detach().double().cpu().numpy() for p in params] for name, (params, _, _) in runs.items()}
    tol = _tolerances(snap["plain"], snap["f64"])
    for name in ("fused", "fused->plain", "plain->fused"):
        for a, b, t in zip(snap[name], snap["f64"], tol):
            print(f"LAMB class {name}: |x - f64| / tolerance {_maxabs(a - b) / t:.3f}")
            assert np.all(np.abs(a - b) <= t), name
    unwritten = _make(False, torch.float64, "cpu")
    _drive(unwritten[1], unwritten[0], range(4), written=False)
    assert _maxabs(unwritten[0][0].detach().numpy() - snap["f64"][0]) > 100 * tol[0]             # the learning-rate writes matter
    # an Adam state loads: counts and moments are taken over, and the next step is a fused one
    adam_params = [torch.nn.Parameter(p.detach().clone()) for p in runs["fused"][0]]
    adam = M.Adam(adam_params, lr=1e-3)
    _drive(adam, adam_params, range(1))
    heir = _make(True)
    sd = copy.deepcopy(adam.state_dict())
    sd["param_groups"] = heir[1].state_dict()["param_groups"]
    heir[1].load_state_dict(sd)
    _drive(heir[1], heir[0], range(2, 3))
    assert all(float(heir[1].state[p]["step"]) == 2.0 and heir[1].state[p]["step"].is_cpu for p in heir[0]) and "_vipant_fused" in vars(heir[1])
