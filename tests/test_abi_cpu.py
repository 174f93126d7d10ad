"""The C ABI: libvipant_hip.so loads (no GPU needed), exports every symbol include/vipant_hip.h declares, the
ctypes table mirrors the header one to one, and the product path refuses CPU tensors instead of falling back."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "vipant_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vipant_\w+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    lib = _ffi.lib()
    syms = header_symbols()
    assert len(syms) >= 28
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/vipant_hip.h but not exported"
    assert sorted(_ffi.PROTOTYPES.keys()) == syms, set(_ffi.PROTOTYPES) ^ set(syms)
    assert _ffi.ABI_VERSION == lib.vipant_version() == 101
    assert lib.vipant_last_error() is not None


def test_library_exports_no_undeclared_symbol():
    """The other direction: every `vipant_*` function the library exports is declared in the header (a forwarder that lost its
    declaration, a debug export outside its #ifdef)."""
    import subprocess
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    exported = {f[-1] for f in map(str.split, out.splitlines()) if f and f[-1].startswith("vipant_")}
    assert len(exported) >= 28
    assert exported <= set(header_symbols()), sorted(exported - set(header_symbols()))


def test_library_of_another_abi_version_is_refused(monkeypatch):
    """Argument lists changed under existing names at version 101: a library that reports another version (VIPANT_HIP_LIB pointing at
    an older build) must be refused before any of its functions can be called."""
    from vipant_amd import _ffi, build
    build.build(verbose=False)
    found = _ffi.lib().vipant_version()
    monkeypatch.setattr(_ffi, "ABI_VERSION", found + 1)
    monkeypatch.setattr(_ffi, "_lib", None)
    with pytest.raises(_ffi.VipantError) as e:
        _ffi.lib()
    assert str(found) in str(e.value) and str(found + 1) in str(e.value) and _ffi.LIB_PATH in str(e.value)
    assert _ffi._lib is None
    monkeypatch.undo()
    assert _ffi.lib().vipant_version() == _ffi.ABI_VERSION


def test_argument_counts_match_header():
    from vipant_amd import _ffi
    text = open(os.path.join(ROOT, "include", "vipant_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, (_, args) in _ffi.PROTOTYPES.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m, name
        params = m.group(1).strip()
        n = 0 if params in ("", "void") else params.count(",") + 1
        assert n == len(args), (name, n, len(args))


def test_workspace_queries_run_without_a_gpu():
    from vipant_amd import _ffi
    assert _ffi.query("vipant_gemm_tn_workspace_bytes", 161792, 3072, 768) == 7 * 36 * 256 * 256 * 4 + 7 * 3 * 12 * 256 * 4
    assert _ffi.query("vipant_infonce_workspace_bytes", 4096, 512) > 4096 * 4096 * 2
    assert _ffi.query("vipant_lars_workspace_bytes", 153) == 153 * 32 * 2 * 4
    assert _ffi.query("vipant_layernorm_bwd_workspace_bytes", 161792, 768) == 256 * 3 * 768 * 4      # one persistent workgroup per CU
    assert _ffi.query("vipant_colsum_workspace_bytes", 1000, 768) == 128 * 768 * 4


def test_bad_arguments_are_reported_not_executed():
    from vipant_amd import _ffi
    with pytest.raises(_ffi.VipantError, match="K%64"):
        _ffi.call("vipant_gemm_nt", 16, 100, 16, 100, 16, 64, None, None, 1.0, 4, 64, 100, 0, None)
    with pytest.raises(_ffi.VipantError, match="empty problem"):
        _ffi.call("vipant_mha_fwd", 16, 16, 16, None, None, 1, 0, 12, 0, None)
    with pytest.raises(_ffi.VipantError, match="16-byte aligned"):
        _ffi.call("vipant_mha_fwd", 8, 16, 16, None, None, 1, 100, 12, 0, None)
    with pytest.raises(_ffi.VipantError, match="workspace"):
        _ffi.call("vipant_infonce_fwd_bwd", 16, 16, 16, 0.0, 16, None, None, None, 1.0, 64, 512, 0, 64, None, 0, None)
    with pytest.raises(_ffi.VipantError, match="K % 128"):
        _ffi.call("vipant_gemm_nt_e4m3", 16, 192, 16, 16, 192, 16, 16, 64, None, None, None, None, 4, 64, 192, 0, None)
    with pytest.raises(_ffi.VipantError, match="block scales of A"):
        _ffi.call("vipant_gemm_nt_e4m3", 16, 256, None, 16, 256, 16, 16, 64, None, None, None, None, 4, 64, 256, 0, None)
    with pytest.raises(_ffi.VipantError, match="go together"):
        _ffi.call("vipant_gemm_nt_e4m3", 16, 256, 16, 16, 256, 16, 16, 64, None, None, 16, None, 4, 64, 256, 0, None)
    with pytest.raises(_ffi.VipantError, match="K % 128"):
        _ffi.call("vipant_quant_e4m3_mx", 16, 192, 16, 192, 16, 4, 192, None)
    assert _ffi.query("vipant_mx_scale_bytes", 323584, 4096) == 323584 * 4096 // 32 and _ffi.query("vipant_mx_scale_bytes", 130, 256) == 2 * 2 * 512
    with pytest.raises(_ffi.VipantError, match="K <= 8192"):
        _ffi.call("vipant_quant_e4m3_rows", 16, 16384, 16, 16384, 16, 4, 16384, None)
    with pytest.raises(_ffi.VipantError, match="go together"):
        _ffi.call("vipant_layernorm_fwd", 16, 768, 16, 16, 16, None, 16, 16, 4, 768, None, None, 16, None, 0, None)


def test_no_cpu_fallback():
    from vipant_amd import _ffi, ops
    a = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(_ffi.VipantError, match="no CPU fallback"):
        ops.gemm_nt(a, a, torch.zeros(4, 4, dtype=torch.bfloat16))
    with pytest.raises(_ffi.VipantError, match="no CPU fallback"):
        ops.InfoNCEFn.apply(torch.zeros(8, 512), torch.zeros(8, 512), torch.zeros(()), 0.0, 0, 8, 1.0)


def test_product_never_imports_the_oracle():
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "vipant_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "ref_cpu" in src:
                    bad.append(os.path.join(dirpath, f))
    for f in ("train.py",):
        if re.search(r"^\s*(from|import)\s+oracle\b", open(os.path.join(ROOT, f)).read(), flags=re.M):
            bad.append(f)
    assert not bad, bad


def test_no_kernel_spills_registers():
    """A spilled accumulator turns a contraction into a scratch-memory kernel without failing any numerics test (it happened once
    in round 2: +25 % on one launch).  The build records clang's per-kernel resource usage; no kernel on the step's path may spill."""
    from vipant_amd import build
    build.build(verbose=False)
    usage = build.resource_usage()
    assert usage.get("gemm_nt.hip") and usage.get("gemm_tn.hip") and usage.get("attention.hip"), list(usage)
    allowed = ("mha_fwd_kernelILi24ELb1E",)              # causal forward at 320 < S <= 384: no tower has that shape
    bad = {k: (u.get("VGPRs Spill"), u.get("ScratchSize [bytes/lane]")) for f, ks in usage.items() for k, u in ks.items()
           if (u.get("VGPRs Spill", 0) or u.get("ScratchSize [bytes/lane]", 0)) and not any(a in k for a in allowed)}
    assert not bad, bad
    n = sum(len(v) for v in usage.values())
    assert n > 200, n


def test_streamed_attention_backward_does_not_touch_v_fragments_before_their_wait():
    """the guard itself lives in vipant_amd/isa_guard.py and runs inside the build, on the assembly of the same compile
    that produced the shipped object (`-save-temps`); here it runs once more on the shipped build."""
    from vipant_amd import build, isa_guard
    build.build(verbose=False)
    isa_guard.check_attention(build.isa_path("attention.hip"))


def test_ticket_walk_mailbox_register_is_never_copied():
    from vipant_amd import build, isa_guard
    build.build(verbose=False)
    isa_guard.check_gemm_nt(build.isa_path("gemm_nt.hip"))


def test_isa_is_from_the_shipped_compile_and_toolchain_is_recorded():
    """The assembly the guards read is a by-product (`-save-temps`) of the compile whose object is linked into the library -- not of a
    second compile -- and the build records which hipcc made it."""
    import json
    from vipant_amd import build
    build.build(verbose=False)
    for name in build.KEEP_ISA:
        s_path, o_path = build.isa_path(name), os.path.join(build.OBJ, name[:-4] + ".o")
        assert os.path.exists(s_path) and os.path.getmtime(s_path) <= os.path.getmtime(o_path) + 1.0, name
    tc = json.load(open(os.path.join(build.OBJ, "toolchain.json")))
    assert "version" in tc and tc["version"], tc


def test_isa_guards_reject_doctored_assembly(tmp_path):
    """The guards must FAIL on assembly that breaks what they guard (they run inside the build: a guard that cannot fail protects
    nothing).  Two edits of the shipped build's own assembly: a copy of the ticket walk's mailbox register right after its asm load
    (what a spill or a relocation by another hipcc would look like), and an instruction that names one of the attention backward's
    in-flight AGPRs before the counted wait."""
    from vipant_amd import build, isa_guard
    build.build(verbose=False)
    text = open(build.isa_path("gemm_nt.hip")).read()
    m = re.search(r"(;+#?ASMSTART\n\s*global_load_dword\s+(v\d+),\s*v\[\d+:\d+\],\s*off\s*\n)", text)
    assert m, "no asm mailbox load found"
    bad = tmp_path / "gemm_nt_bad.s"
    bad.write_text(text.replace(m.group(1), m.group(1) + f"\tv_mov_b32_e32 v1, {m.group(2)}\n", 1))
    with pytest.raises(AssertionError):
        isa_guard.check_gemm_nt(str(bad))
    isa_guard.check_gemm_nt(build.isa_path("gemm_nt.hip"))
    text = open(build.isa_path("attention.hip")).read()
    k = re.search(r"^_ZN\S*mha_bwd1s_kernelILi20ELb0E\S*:", text, flags=re.M)
    body = text[k.start():]
    loads = [x for x in re.finditer(r"global_load_dwordx4\s+a\[(\d+):(\d+)\][^\n]*\n", body)]
    assert len(loads) >= 10
    wait = body.index("s_waitcnt vmcnt(22)")
    last = [x for x in loads if x.end() < wait][-1]
    doctored = text[:k.start()] + body[:last.end()] + f"\tv_accvgpr_read_b32 v1, a{last.group(1)}\n" + body[last.end():]
    bad2 = tmp_path / "attention_bad.s"
    bad2.write_text(doctored)
    with pytest.raises(AssertionError):
        isa_guard.check_attention(str(bad2))
