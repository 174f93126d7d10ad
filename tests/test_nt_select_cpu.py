"""Which kernel instance an NT contraction launch reaches (vipant_amd/csrc/nt_select.h), checked without a GPU: the header is
compiled alone by the host compiler into tests/nt_select_main.cpp and its answers are compared with tests/golden/nt_select_table.txt --
recorded from the dispatch code as it stood before the selector existed (a line-by-line transcription of its four ladders): the
launches of the ViT-B and ViT-L steps (bf16 and e4m3, every emit mode), one launch on each side of every threshold, every switch that
moves a choice, every refusal."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "nt_select_table.txt")


def rows():
    out = []
    for line in open(TABLE):
        if line.strip() and not line.startswith("#"):
            label, launch, expected = (f.strip() for f in line.split("|"))
            out.append((label, launch, expected))
    return out


def test_selector_matches_recorded_table(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "nt_select_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "nt_select_main.cpp")], check=True)
    table = rows()
    got = subprocess.run([exe], input="\n".join(r[1] for r in table) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    assert len(got) == len(table) >= 170
    wrong = [f"{label}: {launch}: selected `{g}`, recorded `{expected}`" for (label, launch, expected), g in zip(table, got) if g != expected]
    assert not wrong, "\n".join(wrong)
    # the anchors of the ViT-B step, spelled out
    by_label = {label: expected for label, _, expected in table}
    assert by_label["vitb qkv bf16"] == "pingpong epi=0 sched=10 es=2 emit=0 ticket=1"          # DEEP, plain walk (nine column tiles), tickets
    assert by_label["vitb c_fc bf16"] == "pingpong epi=6 sched=12 es=2 emit=0 ticket=1"         # DEEP on the column-grouped walk
    assert by_label["vitb c_fc_act_bwd bf16"] == "pingpong epi=7 sched=12 es=2 emit=0 ticket=1"
    assert by_label["vitb out_proj bf16"] == "pingpong epi=0 sched=0 es=2 emit=0 ticket=1"      # k-step schedule
    assert by_label["vitb c_proj bf16"] == "pingpong epi=0 sched=10 es=2 emit=0 ticket=1"


def test_switch_names_agree():
    """vipant_amd/_ffi.py repeats the names of the switches Python code sets: same values as csrc/switches.h."""
    import re
    from vipant_amd import _ffi
    text = open(os.path.join(ROOT, "vipant_amd", "csrc", "switches.h")).read()
    header = {m.group(1): 1 << int(m.group(2)) for m in re.finditer(r"VIPANT_SW_(\w+) = 1 << (\d+)", text)}
    assert len(header) == 15 and len(set(header.values())) == 15
    for name in ("GROUPED_ALWAYS", "GROUPED_NEVER", "STATIC_WALK", "ROUND4_SCHEDULES"):
        assert getattr(_ffi, "SW_" + name) == header[name], name
