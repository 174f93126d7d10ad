"""The CPU half of tests/test_gemm_nt_gpu.py: every case of tests/nt_cases.py reaches the kernel instance it claims (the selector
driver tests/nt_select_main.cpp, compiled by the host compiler as tests/test_nt_select_cpu.py does), every kernel instance listed in
vipant_amd/csrc/gemm_nt.hip is claimed by a case -- every bf16 ping-pong instance on both walks -- and the lists keep every property
they were chosen for.  A kernel added to NT_PP_INSTANCES, NT_PLAIN_INSTANCES or NT_FEW_ROWS_INSTANCES without a parity case fails here."""
import os
import re
import shutil
import subprocess

import pytest

import nt_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vipant_amd", "csrc")


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("nt_cases") / "nt_select_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "nt_select_main.cpp")], check=True)

    def run(lines):
        got = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
        assert len(got) == len(lines)
        return got
    return run


def library_instances():
    """The rows of the three instance lists of gemm_nt.hip, in the driver's words."""
    text = open(os.path.join(CSRC, "gemm_nt.hip")).read()
    header = open(os.path.join(ROOT, "include", "vipant_hip.h")).read()
    epi = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (VIPANT_EPI_\w+) (\d+)\b", header)}
    select_h = open(os.path.join(CSRC, "nt_select.h")).read()
    sched = {m.group(1): int(m.group(2)) for m in re.finditer(r"(NT_(?:KSTEP|DEEP)\w*) = (\d+)", select_h)}
    emit = {m.group(1): int(m.group(2)) for m in re.finditer(r"(NT_EMIT_\w+) = (\d+)", select_h)}
    assert len(sched) == 4 and len(emit) == 4

    def body(name):
        m = re.search(r"#define %s\(X\)((?:[^\n]*\\\n)*[^\n]*)\n" % name, text)
        assert m, name
        return m.group(1)
    pp = [(epi[e], sched[s], int(es), emit[em]) for e, s, es, em in re.findall(r"X\((VIPANT_EPI_\w+), (NT_\w+), (\d), (NT_EMIT_\w+)\)", body("NT_PP_INSTANCES"))]
    plain = [epi[e] for e in re.findall(r"X\((VIPANT_EPI_\w+)\)", body("NT_PLAIN_INSTANCES"))]
    few = [epi[e] for e in re.findall(r"X\((VIPANT_EPI_\w+)\)", body("NT_FEW_ROWS_INSTANCES"))]
    return pp, plain, few


def test_every_case_reaches_the_instance_it_claims(select):
    got = select([C.driver_line(c) for c in C.ALL_CASES])
    wrong = [f"{C.case_id(c)}: selected `{g}`, claimed `{c.inst}`" for c, g in zip(C.ALL_CASES, got) if g != c.inst]
    assert not wrong, "\n".join(wrong)
    assert len(set(C.ALL_CASES)) == len(C.ALL_CASES), "a case is listed twice"
    got = select([C.driver_line(c) for c, _ in C.REFUSALS])
    assert got == [c.inst for c, _ in C.REFUSALS], got
    lines = [C.driver_line(c).split() for c, _, _ in C.MISALIGNED_AUX]
    got = select([" ".join(f[:10] + ["1"] + f[11:]) for f in lines])
    assert got == [refusal for _, refusal, _ in C.MISALIGNED_AUX], got
    # ... and each of those launches is accepted with an aligned aux: the refusal is the pointer's
    assert select([" ".join(f) for f in lines]) == [c.inst for c, _, _ in C.MISALIGNED_AUX]


def claimed(cases):
    return {C.parse_instance(c.inst) for c in cases}


def uncovered(pp, plain, few, cases):
    have = claimed(cases)
    missing = []
    for e, s, es, em in pp:
        for ticket in ((0, 1) if es == 2 else (0,)):
            if ("pingpong", e, s, es, em, ticket) not in have:
                missing.append(C.pp(e, s, es, em, ticket))
    missing += [C.plain(e) for e in plain if ("plain", e, None, None, None, None) not in have]
    missing += [C.few_rows(e) for e in few if ("few_rows", e, None, None, None, None) not in have]
    return missing


def test_every_kernel_instance_of_the_library_has_a_case():
    pp, plain, few = library_instances()
    missing = uncovered(pp, plain, few, C.ALL_CASES)
    assert not missing, "kernel instances without a parity case: " + "; ".join(missing)
    # (the regular expressions found the lists as they stand today: 18 bf16 and 14 e4m3 ping-pong kernels, six plain, five few-rows)
    assert len(pp) == 32 and len(set(pp)) == 32 and len(plain) == 6 and len(few) == 5, (len(pp), plain, few)
    assert sum(1 for r in pp if r[2] == 2) == 18 and sum(1 for r in pp if r[2] == 1) == 14
    # no case claims a kernel the library does not hold
    rows = {("pingpong",) + r for r in pp}
    for c in C.ALL_CASES:
        i = C.parse_instance(c.inst)
        assert (i[:5] in rows) if i[0] == "pingpong" else (i[1] in (plain if i[0] == "plain" else few)), C.case_id(c)
    # the check notices a kernel more in any of the three lists, and a bf16 instance claimed on one walk only
    assert uncovered(pp + [(C.QUICKGELU, C.DEEP_GROUPED, 2, 0)], plain, few, C.ALL_CASES) == [C.pp(3, 12, 2, 0, 0), C.pp(3, 12, 2, 0, 1)]
    assert uncovered(pp, plain + [C.QUICKGELU_D8], few, C.ALL_CASES) == [C.plain(6)]
    assert uncovered(pp, plain, few + [C.SCALE_F32], C.ALL_CASES) == [C.few_rows(5)]
    static_only = [c for c in C.ALL_CASES if not (c.epi == C.QUICKGELU and C.parse_instance(c.inst)[2:] == (C.KSTEP_GROUPED, 2, 0, 1))]
    assert uncovered(pp, plain, few, static_only) == [C.pp(3, 8, 2, 0, 1)]


def test_switch_values_agree_with_the_header():
    text = open(os.path.join(CSRC, "switches.h")).read()
    header = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"VIPANT_SW_(\w+) = 1 << (\d+)", text)}
    for short, name in C.SW_HEADER_NAMES.items():
        assert C.SW[short] == header[name], name
    header_h = open(os.path.join(ROOT, "include", "vipant_hip.h")).read()
    epi = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define VIPANT_EPI_(\w+) (\d+)\b", header_h)}
    for name in ("BF16", "F32", "RESIDUAL_F32", "QUICKGELU", "DQUICKGELU", "SCALE_F32", "QUICKGELU_D8", "DQUICKGELU_D8"):
        assert getattr(C, name) == epi[name], name


def test_case_lists_cover_what_they_were_chosen_for():
    C.check_coverage()
    # the figures the ticket cases were chosen by (qlen_own of gemm_nt_pp_kernel, restated in nt_cases.queue_lengths)
    q = {(c.M, c.N, c.epi): C.queue_lengths(c) for c in C.TICKET_CASES[::2]}
    assert q[(33700, 2048, C.BF16)] == [132] * 8 and q[(58300, 2048, C.BF16)] == [228] * 8
    assert q[(109300, 768, C.QUICKGELU_D8)] == [161] + [160] * 7
    assert q[(108600, 768, C.DQUICKGELU_D8)] == [160] * 7 + [155]
    assert q[(132000, 512, C.QUICKGELU_D8)] == [129] * 8
    assert q[(67228, 1024, C.QUICKGELU_D8)] == [132, 132, 132, 130] * 2
    assert q[(51200, 2304, C.BF16)] == [232] + [224] * 7
    assert all(c.K == 256 for c in C.TICKET_CASES)
    assert max(c.M * c.N for c in C.ALL_CASES) == 58300 * 2048 and max(c.M for c in C.ALL_CASES) == 132000        # 239 MB of bf16 output at most


def _without(cases, pred):
    return [c for c in cases if not pred(c)]


@pytest.mark.parametrize("which,pred", [
    ("ticket", lambda c: (c.M, c.N) == (33700, 2048)),                                  # taper only
    ("ticket", lambda c: (c.M, c.N) == (58300, 2048)),                                  # pairs, then the taper
    ("ticket", lambda c: c.M in (108600, 26800)),                                       # unequal queues (1275 and 1260 tiles)
    ("ticket", lambda c: c.M == 67228),                                                 # short last quarter
    ("ticket", lambda c: c.M == 51200),                                                 # plain walk, pairs in front of the taper
    ("ticket", lambda c: (c.M, c.epi) == (65300, C.BF16) and c.sw & C.STATIC),          # a static twin
    ("static", lambda c: c.K == 576 and c.sw == C.DA),                                  # nine K-tiles on DEEP
    ("static", lambda c: c.K == 1024 and c.sw == C.DN),                                 # sixteen K-tiles on KSTEP
    ("static", lambda c: c.M == 33400 and c.epi == C.BF16),                             # 131 row tiles on KSTEP_GROUPED
    ("static", lambda c: c.M == 33100 and c.epi == C.QUICKGELU_D8),                     # 130 row tiles on DEEP_GROUPED
    ("static", lambda c: c.ldc == 520 and c.epi == C.QUICKGELU_D8),                     # the 16-column path's fallback
    ("static", lambda c: c.ldc == 272 and c.epi == C.QUICKGELU_D8),
    ("static", lambda c: c.N == 1800),
    ("small", lambda c: c.M == 700 and c.epi == C.DQUICKGELU),                          # nine tiles
    ("small", lambda c: c.M == 1 and c.epi == C.QUICKGELU),                             # N = 8
    ("plain_", lambda c: c.K == 1024 and c.epi == C.SCALE_F32),
    ("plain_", lambda c: c.inplace),
    ("plain_", lambda c: c.ldc == 260 and c.epi == C.DQUICKGELU),
    ("few", lambda c: c.K == 1600 and c.epi == C.F32),
    ("few", lambda c: c.M == 65 and c.epi == C.DQUICKGELU_D8),
    ("e4m3", lambda c: (c.M, c.K) == (700, 768) and C.parse_instance(c.inst)[4] == C.EMIT_WITH_CODES),
    ("e4m3", lambda c: c.M == 32600 and c.K == 256 and c.inst == C.pp(7, 8, 1, 2, 0)),
    ("e4m3", lambda c: c.K == 768 and c.sw == C.SW["E4M3_WIDE_PLAIN_WALK"]),
])
def test_coverage_notices_a_lost_case(which, pred):
    cases = getattr(C, {"plain_": "PLAIN", "few": "FEW_ROWS"}.get(which, which.upper()) + "_CASES")
    assert any(pred(c) for c in cases)
    with pytest.raises(AssertionError, match="lost"):
        C.check_coverage(**{which: _without(cases, pred)})
