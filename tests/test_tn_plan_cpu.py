"""The CPU half of tests/test_gemm_tn_gpu.py: the Python restatement of the TN contraction's split plans (tests/tn_plan.py) agrees
with vipant_amd/csrc/tn_plan.h in every field (the header is compiled alone by the host compiler into tests/tn_plan_main.cpp) and with
the library's three workspace queries -- the check that the library uses the header -- on every listed and a few hundred
pseudo-random shapes, and the GPU tests' case lists keep every property they were chosen for."""
import os
import random
import shutil
import subprocess

import pytest

import tn_plan as T


@pytest.fixture(scope="module")
def query():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    return _ffi.query


def shapes():
    rng = random.Random(20261018)
    out = [c[:3] for c in T.BF16_CASES + T.PAIR_CASES + T.E4M3_CASES]
    for _ in range(400):
        M = rng.choice([rng.randint(1, 300), rng.randint(1, 5000), rng.randint(1, 400000)])
        P = rng.choice([rng.randint(1, 600), 128 * rng.randint(1, 40), 8 * rng.randint(1, 2000)])
        Q = rng.choice([4 * rng.randint(1, 150), 128 * rng.randint(1, 40), 4 * rng.randint(1, 4000)])
        out.append((M, P, Q))
    return out


@pytest.mark.parametrize("env", [None, "2", "4"])
def test_restated_plans_agree_with_the_workspace_queries(query, monkeypatch, env):
    if env is None:
        monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    else:
        monkeypatch.setenv("VIPANT_TN_SPLIT", env)
    assert T.split_factor() == int(env or 1)
    seen = set()
    for M, P, Q in shapes():
        for name, fn, pair in (("vipant_gemm_tn_workspace_bytes", T.plan, False), ("vipant_gemm_tn_e4m3_workspace_bytes", T.plan8, False),
                               ("vipant_gemm_tn_pair_workspace_bytes", T.plan_pair, True)):
            l = fn(M, P, Q)
            got = query(name, M, P, Q)
            assert got == l.ws_bytes and T.splits_from_bytes(got, P, Q, pair) == l.splits, (name, env, (M, P, Q), got, l)
            assert 1 <= l.last <= l.per and (l.splits - 1) * l.per + l.last == l.nk and l.parts == l.splits * l.ntq
            seen.add((name, l.splits > 1, l.last < l.per))
    assert len(seen) >= 8, seen          # every query met single and several splits, with and without a short last one


def test_restated_plans_agree_with_the_header_in_every_field(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "tn_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(root, "tests", "tn_plan_main.cpp")], check=True)
    asked, want = [], []
    for M, P, Q in shapes():
        for factor in (1, 2, 4, 8):
            for acc in (0, 1):
                for kind, l in (("bf16", T.plan(M, P, Q, bool(acc), factor)), ("e4m3", T.plan8(M, P, Q, bool(acc), factor)), ("pair", T.plan_pair(M, P, Q))):
                    asked.append(f"{kind} {M} {P} {Q} {factor} {acc}")
                    want.append(f"ntp={l.ntp} ntq={l.ntq} tiles={l.tiles} nk={l.nk} splits={l.splits} per={l.per} direct={int(l.direct)} "
                                f"slab_bytes={l.slab_bytes} colsum_bytes={l.colsum_bytes} workspace_bytes={l.ws_bytes} "
                                f"reduce_blocks={l.reduce_blocks} cs_parts={l.parts} cs_stride={l.cs_stride}")
    got = subprocess.run([exe], input="\n".join(asked) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert len(got) == len(asked) >= 24 * 400
    wrong = [f"{a}: header `{g}`, tests/tn_plan.py `{w}`" for a, g, w in zip(asked, got, want) if g != w]
    assert not wrong, "\n".join(wrong[:20])
    # both sides of what the fields decide: the two reduce-grid caps, direct and slab launches, factors that move the plan and that do not
    plans = [dict(f.split("=") for f in g.split()) for g in got]
    capped = {(a.split()[0], int(p["reduce_blocks"]) == (1024 if a.startswith("pair") else 2048)) for a, p in zip(asked, plans)}
    assert capped == {(k, c) for k in ("bf16", "e4m3", "pair") for c in (False, True)}
    assert {(a.split()[0], p["direct"]) for a, p in zip(asked, plans)} == {(k, d) for k in ("bf16", "e4m3", "pair") for d in "01"}
    assert all(p["colsum_bytes"] == "0" for a, p in zip(asked, plans) if a.startswith("pair"))


def test_split_factor_is_atoi_clamped_to_1_8(monkeypatch):
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    assert T.split_factor() == 1
    for env, want in (("", 1), ("0", 1), ("-3", 1), ("1", 1), ("2", 2), ("4", 4), ("8", 8), ("9", 8), ("3x", 3), ("x", 1), (" 5", 5)):
        assert T.split_factor(env) == want, env
    assert T.plan(833, 2048, 2048, factor=2).splits == 7 and T.plan(833, 2048, 2048, factor=4).per == 1
    assert T.plan(161792, 3072, 768, factor=1).splits == 7          # tests/test_abi_cpu.py's shape
    assert T.plan(1000, 4352, 4352, factor=4).splits == 1          # more than 256 tiles: the factor does not apply


def test_case_lists_cover_what_they_were_chosen_for(monkeypatch):
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    T.check_coverage()
    l = {c[:3]: T.plan(*c[:3]) for c in T.BF16_CASES}
    # the figures the lists were chosen by
    assert all((l[(128 * k, 2304, 2560)].tiles, l[(128 * k, 2304, 2560)].splits, l[(128 * k, 2304, 2560)].per) == (90, 2, k) for k in range(1, 10))
    assert [(l[s].per, l[s].last, l[s].mtail) for s in ((833, 2048, 2048), (447, 2048, 2048), (352, 2048, 2048), (1352, 2048, 2048),
                                                         (1617, 2304, 768))] == [(4, 2, 1), (2, 1, 63), (2, 2, 32), (6, 4, 8), (3, 2, 17)]
    assert (l[(2560, 768, 3072)].tiles, l[(2560, 768, 3072)].ntq, l[(2560, 768, 3072)].parts) == (36, 12, 84)
    assert (l[(200, 3072, 3072)].direct, l[(200, 3072, 3072)].per, l[(200, 3072, 3072)].parts) == (True, 4, 12)
    assert (l[(1000, 3080, 3076)].direct, l[(1000, 3080, 3076)].per, l[(1000, 3080, 3076)].parts) == (True, 16, 13)
    assert [l[(64 * n, 256, 256)].parts for n in (1, 2, 3, 4, 5, 8, 9)] == [1, 2, 3, 4, 5, 8, 9]
    assert all(T.plan_pair(128 * k, 2048, 2048).per == k and T.plan_pair(256 * k, 2048, 2048).per == 2 * k for k in range(1, 8))
    assert all(T.plan8(256 * k, 2304, 2560).per == k for k in range(1, 8))
    assert not T.plan(64, 256, 256, accumulate=True).direct


def _without(cases, *drop):
    return [c for c in cases if c[:3] not in drop]


@pytest.mark.parametrize("drop", [(128 * k, 2304, 2560) for k in (5, 7, 8, 9)] + [
    (833, 2048, 2048), (447, 2048, 2048), (352, 2048, 2048), (200, 3072, 3072), (1000, 3080, 3076), (1, 8, 4), (385, 100, 260),
    (320, 256, 256), (576, 256, 256)])
def test_coverage_notices_a_lost_bf16_case(monkeypatch, drop):
    """Each of these is the only case of its kind: per = 5, 7, 8, 9 (the other K-tile counts have a second case); the fourth short
    (per, last) pair; the only last split of one K-tile; M % 64 = 32; the two direct launches of several K-tiles (parts = 12, 13,
    per = 16); M = 1 and Q = 4; P % 8 != 0 and Q = 260; parts = 5 and 9."""
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    with pytest.raises(AssertionError, match="lost"):
        T.check_coverage(bf16=_without(T.BF16_CASES, drop))


@pytest.mark.parametrize("which,drop", [("pair", (384, 2048, 2048)), ("pair", (896, 2048, 2048)), ("pair", (545, 1024, 1024)),
                                        ("pair", (63, 264, 12)), ("e4m3", (768, 2304, 2560)), ("e4m3", (1792, 2304, 2560)),
                                        ("e4m3", (100, 128, 128))])
def test_coverage_notices_a_lost_pair_or_e4m3_case(monkeypatch, which, drop):
    monkeypatch.delenv("VIPANT_TN_SPLIT", raising=False)
    kw = {which: _without(getattr(T, which.upper() + "_CASES"), drop)}
    with pytest.raises(AssertionError, match="lost"):
        T.check_coverage(**kw)
