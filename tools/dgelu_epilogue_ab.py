"""The QuickGELU' launch of the NT contraction, this build against another build of the same ABI (the parent commit's library):

  python tools/dgelu_epilogue_ab.py hash
        sha256 of the output bytes of seeded launches -- the three shapes of tests/test_nt_dgelu_epilogue_gpu.py and the step's shape,
        codes and bf16 pre-activations, ticket and static walk.  Run it once per library (VIPANT_HIP_LIB=<other build> for the second
        process) and compare the lines: any difference is a bug.
  python tools/dgelu_epilogue_ab.py time <other libvipant_hip.so> [rounds]
        per-launch times of the step's QuickGELU' launch (M = 161 792, N = 3072, K = 768, codes) and of the BF16 launch of the same
        shape (the floor: the same stores, no codes), the two libraries alternating in ONE process, tools/walk_ab.py style."""
import ctypes
import hashlib
import os
import shutil
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vipant_amd import _ffi, ops  # noqa: E402

dev = "cuda:0"
STATIC = _ffi.SW_STATIC_WALK
DEEP_ALWAYS = 1 << 17


def operands(M, N, K, ldc, epi, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    a = (torch.randn(M, K, generator=g, device=dev)).to(torch.bfloat16)
    b = (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(torch.bfloat16)
    if epi == ops.EPI_DQUICKGELU_D8:
        aux = torch.randint(0, 256, (M, ldc), generator=g, device=dev, dtype=torch.uint8)
    else:
        aux = (torch.randn(M, ldc, generator=g, device=dev) * 2).to(torch.bfloat16)
    out = torch.zeros(M, ldc, dtype=torch.bfloat16, device=dev)
    return a, b, aux[:, :N], out[:, :N], out


def cmd_hash():
    shapes = [("tile_wrap", 33000, 1024, 192, 1024, DEEP_ALWAYS), ("grouped_walk", 22400, 3072, 128, 3072, 0), ("edges", 300, 264, 128, 304, 0),
              ("step", 512 * 316, 3072, 768, 3072, 0)]
    for name, M, N, K, ldc, sw in shapes:
        for epi, ename in ((ops.EPI_DQUICKGELU_D8, "codes"), (ops.EPI_DQUICKGELU, "bf16u")):
            a, b, aux, out, parent = operands(M, N, K, ldc, epi, M * 31 + N + epi)
            for walk, wname in ((0, "ticket"), (STATIC, "static")):
                os.environ["VIPANT_GEMM_VARIANT"] = str(sw | walk)
                parent.zero_()
                ops.gemm_nt(a, b, out, aux=aux, epi=epi)
                torch.cuda.synchronize()
                h = hashlib.sha256(parent.cpu().view(torch.int16).numpy().tobytes()).hexdigest()
                print(f"{name:12s} {M:6d} x {N:4d} x {K:3d} ldc {ldc:4d} {ename} {wname}: {h}", flush=True)
            del a, b, aux, out, parent
    os.environ.pop("VIPANT_GEMM_VARIANT", None)


def load_other(path):
    """A second handle with the prototypes attached (a private copy of the file: the loader would hand back the first handle for a path
    it already holds)."""
    tmp = os.path.join(tempfile.mkdtemp(), "libvipant_other.so")
    shutil.copy(path, tmp)
    handle = ctypes.CDLL(tmp)
    assert handle.vipant_version() == _ffi.ABI_VERSION
    for name, (res, args) in _ffi.PROTOTYPES.items():
        if hasattr(handle, name):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
    return handle


def cmd_time(other_path, rounds):
    libs = {"this": _ffi.lib(), "other": load_other(other_path)}
    M, N, K = 512 * 316, 3072, 768
    a, b, aux, out, _ = operands(M, N, K, N, ops.EPI_DQUICKGELU_D8, 1)
    cases = [("dgelu8 N=3072 K=768", lambda: ops.gemm_nt(a, b, out, aux=aux, epi=ops.EPI_DQUICKGELU_D8)),
             ("bf16   N=3072 K=768", lambda: ops.gemm_nt(a, b, out, epi=ops.EPI_BF16))]

    def one(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for walk, wname in ((0, "ticket"), (STATIC, "static")):
        os.environ["VIPANT_GEMM_VARIANT"] = str(walk)
        for name, fn in cases:
            t = {k: [] for k in libs}
            for k, h in libs.items():
                _ffi._lib = h
                fn(); fn()
            torch.cuda.synchronize()
            for _ in range(rounds):
                for k, h in libs.items():
                    _ffi._lib = h
                    t[k].append(one(fn))
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            print(f"{name} {wname}: " + "   ".join(f"{k} median {med[k]:7.1f} us (min {min(v):7.1f}, max {max(v):7.1f})" for k, v in t.items())
                  + f"   this - other {med['this'] - med['other']:+6.1f} us", flush=True)
    _ffi._lib = libs["this"]
    os.environ.pop("VIPANT_GEMM_VARIANT", None)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "hash":
        cmd_hash()
    elif len(sys.argv) >= 3 and sys.argv[1] == "time":
        cmd_time(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 15)
    else:
        sys.exit(__doc__)
