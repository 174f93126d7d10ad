"""Tensor-level wrappers over the C ABI plus the autograd nodes of the contrastive step.

PyTorch is plumbing here: it owns device memory, streams and the autograd tape; every numeric
operation below is a call into libvipant_hip.so (hand-written gfx950 kernels).  Nothing in this file
computes on the CPU or through ATen kernels, except zero-fills / views used as allocation helpers.

Activation layout: token-major [M, D] with M = batch * tokens, row m = b * S + s (batch-first).
The residual stream and its gradient are fp32; every MFMA operand is bf16 (fp32 accumulate).
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _ffi
from ._ffi import (EPI_BF16, EPI_DQUICKGELU, EPI_DQUICKGELU_D8, EPI_F32, EPI_QUICKGELU, EPI_QUICKGELU_D8,  # noqa: F401
                   EPI_RESIDUAL_F32, EPI_SCALE_F32,
                   call, query)

BF16, F32, F16, I64 = torch.bfloat16, torch.float32, torch.float16, torch.int64

# order of the 12 per-layer parameters handed to BackboneFn (reference names, cvap/module/val.py:496-507)
BLOCK_PARAM_NAMES = (
    "ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias",
    "attn.out_proj.weight", "attn.out_proj.bias", "ln_2.weight", "ln_2.bias",
    "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias",
)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _need(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _ffi.VipantError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise _ffi.VipantError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t.stride(-1) != 1 and t.numel() > 1:
        raise _ffi.VipantError(f"{name}: last dimension must be contiguous")


def no_tape(params):
    """Parameters as the autograd nodes below should see them: under torch.no_grad() (Monitor.infer, cfg.eval) nothing
    will be differentiated, but `ctx.needs_input_grad` still reports `requires_grad` -- and `forward` itself always runs
    with grad mode off, so it cannot tell.  Detached parameters make the nodes take their forward-only path (one set of
    temporaries for all layers, cached bf16 weights, nothing saved)."""
    return params if torch.is_grad_enabled() else tuple(p.detach() for p in params)


_scratch: Dict[Tuple[str, int], torch.Tensor] = {}

# bench.py hooks a probe here to bracket selected kernel launches with HIP events on the launch stream
# (kernels are launched on torch's current stream, so torch.cuda.Event records on the right queue).
KERNEL_PROBE: Dict[str, dict] = {}


def scratch(name: str, nbytes: int, device) -> torch.Tensor:
    """Named, grow-only byte workspace (256-B aligned by the caching allocator)."""
    key = (name, device.index if device.index is not None else torch.cuda.current_device())
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _scratch[key] = buf
    return buf


# --------------------------------------------------------------------------------------- raw ops
def gemm_nt(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, *, bias=None, aux=None, epi: int = EPI_BF16,
            alpha: float = 1.0, few_rows: bool = False):
    """c[M,N] = a[M,K] @ b[N,K]^T with the epilogue `epi` (see include/vipant_hip.h).  `few_rows`: the rows are one per item of a
    batch (VIPANT_EPI_FEW_ROWS: small tiles, K split over a workgroup's waves)."""
    _need(a, BF16, "gemm_nt.a"); _need(b, BF16, "gemm_nt.b")
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and tuple(c.shape) == (M, N), (a.shape, b.shape, c.shape)
    if aux is not None:
        assert aux.stride(0) == c.stride(0)
    probe = KERNEL_PROBE.get("gemm_nt")
    if probe is not None and probe["match"](epi, M, N, K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    else:
        probe = None
    call("vipant_gemm_nt", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0),
         _ptr(bias), _ptr(aux), float(alpha), M, N, K, epi | (_ffi.EPI_FEW_ROWS if few_rows else 0), _stream())
    if probe is not None:
        e1.record()
        probe["events"].append((e0, e1))
    return c


def _stats(n: int, device):
    """(mean, rstd) of a normalisation over n rows (or columns): fp32 [n] each."""
    return torch.empty((n,), dtype=F32, device=device), torch.empty((n,), dtype=F32, device=device)


def mx_buffer(M: int, cols: int, device):
    """(uint8 [M, cols], uint8 [vipant_mx_scale_bytes(M, cols)]): room for an e4m3 operand and its block scales in the MX layout."""
    return (torch.empty((M, cols), dtype=torch.uint8, device=device),
            torch.empty((query("vipant_mx_scale_bytes", M, cols),), dtype=torch.uint8, device=device))


def quant_e4m3(x: torch.Tensor, q: torch.Tensor = None, scale: torch.Tensor = None):
    """bf16 rows [M, K] -> (e4m3 bytes [M, K], E8M0 row-scale bytes [M]); see vipant_quant_e4m3_rows."""
    _need(x, BF16, "quant_e4m3.x")
    M, K = x.shape
    if q is None:
        q = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    if scale is None:
        scale = torch.empty((M,), dtype=torch.uint8, device=x.device)
    call("vipant_quant_e4m3_rows", x.data_ptr(), x.stride(0), q.data_ptr(), q.stride(0), scale.data_ptr(), M, K, _stream())
    return q, scale


def quant_e4m3_mx(x: torch.Tensor, q: torch.Tensor = None, scale: torch.Tensor = None):
    """bf16 rows [M, K] -> (e4m3 bytes [M, K], E8M0 BLOCK scales, one per 32 elements of a row, in the library's MX layout:
    vipant_quant_e4m3_mx) -- the form an activation operand of gemm_nt_e4m3 takes.  q, scale: both or neither."""
    _need(x, BF16, "quant_e4m3_mx.x")
    M, K = x.shape
    if q is None and scale is None:
        q, scale = mx_buffer(M, K, x.device)
    call("vipant_quant_e4m3_mx", x.data_ptr(), x.stride(0), q.data_ptr(), q.stride(0), scale.data_ptr(), M, K, _stream())
    return q, scale


def quant_e4m3_mx32(x: torch.Tensor, q: torch.Tensor = None, scale: torch.Tensor = None):
    """bf16 rows [M, K] -> (e4m3 bytes, block scales in the MX layout) with every scale shared by an aligned block of 32 rows x 32
    columns (vipant_quant_e4m3_mx32): an operand of gemm_tn_e4m3, a valid activation operand of gemm_nt_e4m3.  q, scale: both or neither."""
    _need(x, BF16, "quant_e4m3_mx32.x")
    M, K = x.shape
    if q is None and scale is None:
        q, scale = mx_buffer(M, K, x.device)
    call("vipant_quant_e4m3_mx32", x.data_ptr(), x.stride(0), q.data_ptr(), q.stride(0), scale.data_ptr(), M, K, _stream())
    return q, scale


def mx_uniform32(q: torch.Tensor, scale: torch.Tensor):
    """In place: e4m3 bytes [M, K] with row-wise block scales -> block-uniform scales (vipant_mx_uniform32)."""
    assert q.dtype == torch.uint8 and scale.dtype == torch.uint8 and q.dim() == 2
    M, K = q.shape
    assert scale.numel() >= query("vipant_mx_scale_bytes", M, K)
    call("vipant_mx_uniform32", q.data_ptr(), q.stride(0), scale.data_ptr(), M, K, _stream())
    return q, scale


def gemm_tn_e4m3(a, sa, b, sb, c: torch.Tensor, accumulate: bool = False, a_colsum=None, ws_name: str = "gemm_tn"):
    """c[P, Q] (fp32) (+)= dequant(a, sa)^T @ dequant(b, sb): a [M, P], b [M, Q] e4m3 bytes with block-uniform scales;
    a_colsum (fp32 [P], optional) (+)= column sums of dequant(a, sa)."""
    assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and sa.dtype == torch.uint8 and sb.dtype == torch.uint8
    _need(c, F32, "gemm_tn_e4m3.c")
    M, P = a.shape
    Q = b.shape[1]
    assert b.shape[0] == M and tuple(c.shape) == (P, Q), (a.shape, b.shape, c.shape)
    ws = scratch(ws_name, query("vipant_gemm_tn_e4m3_workspace_bytes", M, P, Q), a.device)
    call("vipant_gemm_tn_e4m3", a.data_ptr(), a.stride(0), sa.data_ptr(), b.data_ptr(), b.stride(0), sb.data_ptr(), c.data_ptr(),
         c.stride(0), M, P, Q, int(accumulate), _ptr(a_colsum), ws.data_ptr(), ws.numel(), _stream())
    return c


def mx_scale_index(M: int, K: int, device) -> torch.Tensor:
    """int64 [M, K // 32]: where the MX layout keeps the scale byte of (row, 32-element block) -- for tests and tools."""
    m = torch.arange(M, device=device).view(M, 1)
    kb = torch.arange(K // 32, device=device).view(1, K // 32)
    return (((m >> 7) * (K // 128) + (kb >> 2)) * 16 + (m & 15)) * 32 + (kb & 3) * 8 + ((m >> 4) & 7)


def gemm_nt_e4m3(a, sa, b, sb, c: Optional[torch.Tensor], *, bias=None, aux=None, epi: int = EPI_BF16, emit=None):
    """c[M,N] (bf16) = dequant(a, sa) @ dequant(b, sb)^T with the epilogue `epi`: e4m3 operands; sa: a's block scales (quant_e4m3_mx),
    sb: b's row scales (quant_e4m3).  emit = (bytes [M, N], block scales): the epilogue also leaves the e4m3 form of its result there;
    c (and aux) may then be None (QuickGELU epilogue)."""
    assert a.dtype == torch.uint8 and b.dtype == torch.uint8 and sa.dtype == torch.uint8 and sb.dtype == torch.uint8
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and sa.numel() >= query("vipant_mx_scale_bytes", M, K) and sb.numel() == N, (a.shape, b.shape, sa.shape)
    assert c is None or tuple(c.shape) == (M, N)
    if aux is not None and c is not None:
        assert aux.stride(0) == c.stride(0)
    call("vipant_gemm_nt_e4m3", a.data_ptr(), a.stride(0), sa.data_ptr(), b.data_ptr(), b.stride(0), sb.data_ptr(), _ptr(c),
         c.stride(0) if c is not None else N, _ptr(bias), _ptr(aux), emit[0].data_ptr() if emit else None,
         emit[1].data_ptr() if emit else None, M, N, K, epi, _stream())
    return c


def gemm_tn(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, accumulate: bool = False, a_colsum=None,
            ws_name: str = "gemm_tn"):
    """c[P,Q] (+)= a[M,P]^T @ b[M,Q] (fp32 out); a_colsum (fp32 [P], optional) (+)= column sums of a.
    `ws_name`: the split-K workspace is shared by all calls of one name -- calls issued on different streams need their own."""
    _need(a, BF16, "gemm_tn.a"); _need(b, BF16, "gemm_tn.b"); _need(c, F32, "gemm_tn.c")
    M, P = a.shape
    Q = b.shape[1]
    assert b.shape[0] == M and tuple(c.shape) == (P, Q), (a.shape, b.shape, c.shape)
    nbytes = query("vipant_gemm_tn_workspace_bytes", M, P, Q)
    ws = scratch(ws_name, nbytes, a.device)
    call("vipant_gemm_tn", a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0), M, P, Q,
         int(accumulate), _ptr(a_colsum), ws.data_ptr(), ws.numel(), _stream())
    return c


def colsum(x: torch.Tensor, out: torch.Tensor, accumulate: bool = False):
    _need(x, BF16, "colsum.x"); _need(out, F32, "colsum.out")
    M, N = x.shape
    ws = scratch("colsum", query("vipant_colsum_workspace_bytes", M, N), x.device)
    call("vipant_colsum_bf16", x.data_ptr(), x.stride(0), out.data_ptr(), M, N, int(accumulate), ws.data_ptr(),
         ws.numel(), _stream())
    return out


def layernorm_fwd(x: torch.Tensor, gamma, beta, *, want_bf16=True, want_f32=False, rows: Optional[int] = None,
                  ldx: Optional[int] = None, add: Optional[torch.Tensor] = None, want_sum=False, sum_f16=False):
    """x fp32 | fp16 [M, D] (or `rows` rows with stride `ldx`) -> (y_bf16 | None, y_f32 | None, mean, rstd[, x + add]).
    `add` (bf16 [M, D]) fuses the block's residual add in front of the norm; want_sum returns the new stream (fp16 with sum_f16)."""
    _need(x, x.dtype if x.dtype == F16 else F32, "layernorm_fwd.x")
    D = x.shape[-1]
    M = rows if rows is not None else x.shape[0]
    ldx = ldx if ldx is not None else x.stride(0)
    y = torch.empty((M, D), dtype=BF16, device=x.device) if want_bf16 else None
    y32 = torch.empty((M, D), dtype=F32, device=x.device) if want_f32 else None
    mean, rstd = _stats(M, x.device)
    xsum = torch.empty((M, D), dtype=F16 if sum_f16 else F32, device=x.device) if (add is not None and want_sum) else None
    flags = (_ffi.STREAM_IN_F16 if x.dtype == F16 else 0) | (_ffi.STREAM_OUT_F16 if sum_f16 else 0)
    call("vipant_layernorm_fwd", x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), _ptr(y), _ptr(y32),
         mean.data_ptr(), rstd.data_ptr(), M, D, _ptr(add), _ptr(xsum), None, None, flags, _stream())
    if add is not None:
        return y, y32, mean, rstd, xsum
    return y, y32, mean, rstd


def residual_add(x: torch.Tensor, add: torch.Tensor) -> torch.Tensor:
    """fp32 out = x (fp32 or fp16 stream) + add (bf16)."""
    out = torch.empty(x.shape, dtype=F32, device=x.device)
    call("vipant_residual_add", x.data_ptr(), add.data_ptr(), out.data_ptr(), x.numel(),
         _ffi.STREAM_IN_F16 if x.dtype == F16 else 0, _stream())
    return out


def gather_rows(x: torch.Tensor, idx: Optional[torch.Tensor], batch: int, S: int) -> torch.Tensor:
    """x [batch * S, D] (any 2- or 4-byte dtype) -> its rows i * S + idx[i] (idx None: the first row of every item), [batch, D]."""
    assert x.dim() == 2 and x.is_contiguous() and x.shape[0] == batch * S
    out = torch.empty((batch, x.shape[1]), dtype=x.dtype, device=x.device)
    call("vipant_gather_rows_bytes", x.data_ptr(), _ptr(idx), out.data_ptr(), batch, S, x.shape[1] * x.element_size(), _stream())
    return out


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, mean, rstd, gamma, *, dres=None, dx=None, lddx=None,
                  dx_bf16=None, dgamma, dbeta, dx_colsum=None, accumulate=False, rows=None, ldx=None):
    D = x.shape[-1]
    M = rows if rows is not None else x.shape[0]
    ldx = ldx if ldx is not None else x.stride(0)
    lddx = lddx if lddx is not None else (dx.stride(0) if dx is not None else D)
    ws = scratch("ln_bwd", query("vipant_layernorm_bwd_workspace_bytes", M, D), x.device)
    call("vipant_layernorm_bwd", dy.data_ptr(), int(dy.dtype == F32) | (_ffi.LN_X_F16 if x.dtype == F16 else 0), x.data_ptr(), ldx, mean.data_ptr(),
         rstd.data_ptr(), gamma.data_ptr(), _ptr(dres), _ptr(dx), lddx, _ptr(dx_bf16), dgamma.data_ptr(),
         dbeta.data_ptr(), _ptr(dx_colsum), int(accumulate), M, D, ws.data_ptr(), ws.numel(), None, None, _stream())


def mha_fwd(qkv: torch.Tensor, batch: int, S: int, H: int, causal: bool, q8=None):
    """q8 = (bytes, block scales): also leave the e4m3 form of `out` there (vipant_quant_e4m3_mx of it, rows of H * 64 bytes)."""
    _need(qkv, BF16, "mha_fwd.qkv")
    out = torch.empty((batch * S, H * 64), dtype=BF16, device=qkv.device)
    lse = torch.empty((batch, H, S), dtype=F32, device=qkv.device)
    oq, oscale = q8 if q8 is not None else (None, None)
    call("vipant_mha_fwd", qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), _ptr(oq), _ptr(oscale), batch, S, H, int(causal), _stream())
    return out, lse


def mha_bwd(qkv, out, dout, lse, batch: int, S: int, H: int, causal: bool, q8=None):
    """q8 = (bytes, block scales): also leave the e4m3 form of `dqkv` there (rows of 3 * H * 64 bytes)."""
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    gq, gscale = q8 if q8 is not None else (None, None)
    call("vipant_mha_bwd", qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(),
         _ptr(gq), _ptr(gscale), batch, S, H, int(causal), _stream())
    return dqkv


def cast_bf16(w: torch.Tensor, transpose: bool = False):
    """fp32 matrix -> (bf16 copy, bf16 transposed copy | None)."""
    _need(w, F32, "cast_bf16.w")
    w2 = w.reshape(w.shape[0], -1) if w.dim() != 2 else w
    assert w2.is_contiguous()
    R, Cc = w2.shape
    dst = torch.empty((R, Cc), dtype=BF16, device=w.device)
    dst_t = torch.empty((Cc, R), dtype=BF16, device=w.device) if transpose else None
    call("vipant_cast_bf16", w2.data_ptr(), dst.data_ptr(), _ptr(dst_t), R, Cc, _stream())
    return dst, dst_t


def cast_bf16_flat(x: torch.Tensor) -> torch.Tensor:
    _need(x, F32, "cast_bf16_flat.x")
    assert x.is_contiguous() and x.numel() % 4 == 0
    dst = torch.empty(x.shape, dtype=BF16, device=x.device)
    call("vipant_cast_bf16", x.data_ptr(), dst.data_ptr(), None, 1, x.numel(), _stream())
    return dst


class _WeightCaster:
    """bf16 copies (W and W^T) of a list of fp32 weight matrices, refreshed by ONE launch (vipant_cast_bf16_multi).  The output
    buffers and the device pointer tables are built once per parameter set and reused every step."""

    def __init__(self, weights: Sequence[torch.Tensor]):
        dev = weights[0].device
        self.key = tuple(w.data_ptr() for w in weights)
        self.keep = [w.untyped_storage() for w in weights]       # the addresses stay ours while this entry lives
        shapes = [(w.shape[0], w.numel() // w.shape[0]) for w in weights]
        self.wb = [torch.empty(s, dtype=BF16, device=dev) for s in shapes]
        self.wt = [torch.empty((s[1], s[0]), dtype=BF16, device=dev) for s in shapes]
        starts = [0]
        for r, c in shapes:
            starts.append(starts[-1] + ((r + 63) // 64) * ((c + 63) // 64))
        self.total = starts[-1]
        self.src = torch.tensor([w.data_ptr() for w in weights], dtype=I64, device=dev)
        self.dst = torch.tensor([t.data_ptr() for t in self.wb], dtype=I64, device=dev)
        self.dst_t = torch.tensor([t.data_ptr() for t in self.wt], dtype=I64, device=dev)
        self.R = torch.tensor([s[0] for s in shapes], dtype=torch.int32, device=dev)
        self.C = torch.tensor([s[1] for s in shapes], dtype=torch.int32, device=dev)
        self.starts = torch.tensor(starts, dtype=torch.int32, device=dev)
        self.n = len(weights)

    def refresh(self):
        call("vipant_cast_bf16_multi", self.src.data_ptr(), self.dst.data_ptr(), self.dst_t.data_ptr(), self.R.data_ptr(),
             self.C.data_ptr(), self.starts.data_ptr(), self.n, self.total, _stream())
        return self.wb, self.wt

    def refresh_e4m3(self):
        """Row-quantised e4m3 copies of the bf16 W and W^T just refreshed: [(bytes, row scales)] per matrix, both orientations
        (the forward contractions read W rows, the input-gradient ones W^T rows)."""
        if not hasattr(self, "wq"):
            dev = self.wb[0].device
            self.wq = [(torch.empty(t.shape, dtype=torch.uint8, device=dev), torch.empty((t.shape[0],), dtype=torch.uint8, device=dev))
                       for t in self.wb]
            self.wtq = [(torch.empty(t.shape, dtype=torch.uint8, device=dev), torch.empty((t.shape[0],), dtype=torch.uint8, device=dev))
                        for t in self.wt]
        for src, (q, sc) in zip(self.wb + self.wt, self.wq + self.wtq):
            quant_e4m3(src, q, sc)
        return self.wq, self.wtq


_casters: Dict[tuple, _WeightCaster] = {}


def cast_weights(weights: Sequence[torch.Tensor], e4m3: bool = False):
    """(list of bf16 W, list of bf16 W^T) for the trainable matrices of a tower, one launch; with `e4m3` also their row-quantised
    e4m3 forms (lists of (bytes, row scales))."""
    key = tuple(w.data_ptr() for w in weights)
    c = _casters.get(key)
    if c is None:
        while len(_casters) >= 16:
            _casters.pop(next(iter(_casters)))
        c = _casters[key] = _WeightCaster([w.detach() for w in weights])
    wb, wt = c.refresh()
    if e4m3:
        return (wb, wt) + tuple(c.refresh_e4m3())
    return wb, wt


FP8_TN = os.environ.get("VIPANT_FP8_TN", "1") != "0"      # e4m3 towers: the weight-gradient contractions on e4m3 operands too (0: bf16, the round-5 form)


def fp8_plan(w=None, w2=None, act=None, dyq=None, emit=None, tn=False, keep=None, keep2=None):
    """struct vipant_fp8_plan for one fused-operator call: w / w2 = (bytes, row scales) of the operator's weights, act = (scratch
    bytes [M, 4D], its block scales), emit = the same pair for the e4m3 form an MLP operator's first contraction leaves for its
    second, dyq = (bytes [M, D], block scales): the quantised stream gradient that travels between the backward operators;
    tn: the operator's weight-gradient contractions run on e4m3 operands; keep / keep2: block-uniform e4m3 forms of its kept forward
    activations."""
    from ._ffi import Fp8Plan
    return Fp8Plan(w[0].data_ptr(), w[1].data_ptr(), w2[0].data_ptr() if w2 else None, w2[1].data_ptr() if w2 else None,
                   act[0].data_ptr(), act[1].data_ptr(), emit[0].data_ptr() if emit else None, emit[1].data_ptr() if emit else None,
                   dyq[0].data_ptr() if dyq else None, dyq[1].data_ptr() if dyq else None, int(bool(tn)),
                   keep[0].data_ptr() if keep else None, keep[1].data_ptr() if keep else None,
                   keep2[0].data_ptr() if keep2 else None, keep2[1].data_ptr() if keep2 else None)


def fp8_scratch(M: int, D: int, device):
    """(bytes [M, 4D], block scales) for an e4m3 activation operand of up to 4 D columns."""
    return mx_buffer(M, 4 * D, device)


_frozen_cache: Dict[tuple, tuple] = {}


def cached_bf16(w: torch.Tensor, transpose_only: bool = False):
    """bf16 copy of a frozen weight, cached until the tensor is modified (frozen towers, eval).

    Keyed by address + version + shape; every entry also holds the source's storage, so the address cannot be handed
    to another tensor while the entry is alive (a freed tower's weights would otherwise alias a later model's)."""
    key = (w.data_ptr(), w._version, tuple(w.shape), transpose_only)
    hit = _frozen_cache.get(key)
    if hit is None:
        # an updated weight (the optimizer bumps its version): drop the copies made from its earlier values
        for stale in [k for k in _frozen_cache if k[0] == key[0] and k[2:] == key[2:] and k[1] != key[1]]:
            _frozen_cache.pop(stale)
        while len(_frozen_cache) >= 1024:
            _frozen_cache.pop(next(iter(_frozen_cache)))
        hit = (cast_bf16(w.detach(), transpose=transpose_only), w.untyped_storage())
        _frozen_cache[key] = hit
    return hit[0][1] if transpose_only else hit[0][0]


# ---------------------------------------------------------------------------------- node-to-node gradient hand-off
# The three autograd nodes of a tower (patch embedding -> transformer stack -> read-out) exchange the residual stream as fp32
# tensors, and autograd wants each node's input gradient as a dense fp32 tensor of that shape: for the read-out that is a
# [M, D] matrix of zeros with `batch` non-zero rows (a 497 MB fill + a cast back to bf16 at cfg2), for the stack a bf16 -> fp32
# cast that the patch embedding's LayerNorm backward immediately undoes.  When a node finds its neighbour in the autograd graph,
# it hands the compact form over directly (an attribute on the neighbour's ctx) and returns a zero-stride placeholder of the
# right shape; the receiver uses the hand-off only if what autograd delivers IS that placeholder -- the very allocation the sender
# made, checked by address, not by shape (another consumer of the same tensor makes autograd sum real gradients into a new tensor,
# and the dense path takes over, with the hand-off added in).  Guards (round 4): a tensor that retains its gradient or
# carries hooks at forward time is never handed around (the hook would see zeros); a hand-off the receiver never consumed -- a
# partial backward over the sender only -- is dropped by the sender's next backward instead of being added a second time; the
# sender keeps its link to the receiver across backward calls (retain_graph).  Hooks registered on the stream AFTER the forward
# cannot be seen from here: they observe the placeholder (zeros); VIPANT_NODE_HANDOFF=0 gives dense gradients everywhere.
_VIEW_NODES = ("ViewBackward0", "ReshapeAliasBackward0", "UnsafeViewBackward0", "AliasBackward0", "ViewBackward1")


NODE_HANDOFF = os.environ.get("VIPANT_NODE_HANDOFF", "1") != "0"     # 0: dense fp32 gradients between the nodes (tests, A/B)


def _producer(t: torch.Tensor, kind: str):
    """The custom node of `kind` that produced `t` (looking through view / reshape nodes), or None."""
    if not NODE_HANDOFF:
        return None
    if getattr(t, "retains_grad", False) or getattr(t, "_backward_hooks", None):
        return None                                  # somebody watches this tensor's gradient: keep it dense
    node = t.grad_fn
    for _ in range(4):
        if node is None:
            return None
        if getattr(node, "_vipant_kind", None) == kind:
            return node
        if type(node).__name__ not in _VIEW_NODES or not node.next_functions:
            return None
        node = node.next_functions[0][0]
    return None


_consts: Dict[Tuple[str, int], torch.Tensor] = {}


def _const(name: str, value: float, device) -> torch.Tensor:
    """A 0-dim fp32 constant per device, created once (every `torch.zeros(())` / `ones_like(loss)` inside the step is a fill launch
    on a dependent chain)."""
    key = (name, device.index if device.index is not None else torch.cuda.current_device())
    t = _consts.get(key)
    if t is None:
        t = _consts[key] = torch.full((), value, dtype=F32, device=device)
    return t


def unit_grad(device) -> torch.Tensor:
    """d loss / d loss = 1 as a cached tensor: `loss.backward(gradient=ops.unit_grad(dev))` saves autograd's `ones_like` fill, and
    InfoNCEFn.backward recognises it (by address) and skips the two multiplications by 1."""
    return _const("one", 1.0, torch.device(device))


def _placeholder(shape, device) -> torch.Tensor:
    # ONE zero scalar per device serves every hand-off: the receiver only asks "is this the 4-byte allocation seen through zero
    # strides?", and a gradient autograd has summed from several consumers never is
    return _const("zero", 0.0, torch.device(device)).expand(*shape)


def _is_placeholder(t: torch.Tensor, ph: torch.Tensor) -> bool:
    """`t` is the placeholder `ph` a neighbour returned to autograd: the same 4-byte allocation seen through zero strides (autograd
    may re-wrap the tensor on the way; it cannot give another tensor this address while `ph` is alive)."""
    return ph is not None and t.dim() == 2 and t.stride() == (0, 0) and t.data_ptr() == ph.data_ptr()


# ---------------------------------------------------------------------------------- patch embedding
class PatchEmbedFn(torch.autograd.Function):
    """ViTPreEncoder.forward (cvap/module/val.py:228-259): patch conv as im2col + MFMA contraction, cls token,
    positional table, ln_pre -- vipant_patch_embed_ln_{fwd,bwd}.  x fp32 [b, C, T, F] -> residual stream fp32 [b*S, D]."""

    @staticmethod
    def forward(ctx, x, conv_w, cls, pos, ln_w, ln_b, stride):
        _need(x, F32, "patch_embed.x")
        x = x.contiguous()
        b, Cx, T, Fq = x.shape
        D, Cw, ph, pw = conv_w.shape
        sh, sw = int(stride[0]), int(stride[1])
        nrow, ncol = (T - ph) // sh + 1, (Fq - pw) // sw + 1
        P, S = nrow * ncol, nrow * ncol + 1
        assert pos.shape[0] >= S, f"positional table has {pos.shape[0]} rows, need {S}"
        # cvap/module/val.py:236-244: non-RGB input with a multi-channel kernel -> channel-mean kernel
        mean_ch = Cx != 3 and Cx != Cw
        assert mean_ch or Cx == Cw, f"input has {Cx} channels, kernel {Cw}"
        kcols = (1 if mean_ch else Cw) * ph * pw
        dev = x.device
        w_eff = torch.empty((D, kcols), dtype=BF16, device=dev)
        patches = torch.empty((b * P, kcols), dtype=BF16, device=dev)
        tok = torch.empty((b * S, D), dtype=F32, device=dev)
        out = torch.empty((b * S, D), dtype=F32, device=dev)
        mean, rstd = _stats(b * S, dev)
        call("vipant_patch_embed_ln_fwd", x.data_ptr(), conv_w.detach().contiguous().data_ptr(),
             cls.detach().contiguous().data_ptr(), pos.detach().contiguous().data_ptr(), ln_w.detach().data_ptr(),
             ln_b.detach().data_ptr(), w_eff.data_ptr(), patches.data_ptr(), tok.data_ptr(), out.data_ptr(),
             mean.data_ptr(), rstd.data_ptr(), b, Cx, T, Fq, D, Cw, ph, pw, sh, sw, int(mean_ch), _stream())
        ctx.save_for_backward(patches, tok, mean, rstd, ln_w)
        ctx.meta = (b, P, D, Cw, ph * pw, mean_ch, tuple(conv_w.shape), tuple(pos.shape))
        ctx._vipant_kind = "patch"
        ctx.stream_grad = None          # the stack's bf16 stream gradient, handed over by BackboneFn.backward
        return out

    @staticmethod
    def backward(ctx, dout):
        patches, tok, mean, rstd, ln_w = ctx.saved_tensors
        b, P, D, Cw, khw, mean_ch, conv_shape, pos_shape = ctx.meta
        dev = dout.device
        handed, ctx.stream_grad = ctx.stream_grad, None
        dout_bf16 = handed is not None and _is_placeholder(dout, handed[1])
        if dout_bf16:
            dout = handed[0]
        else:
            dout = dout.contiguous()
            if handed is not None:      # another consumer of the stream contributed a real gradient: add the stack's to it
                dout = dout + handed[0].to(F32)
        kcols = patches.shape[1]
        dtok = torch.empty_like(tok)
        dpatch = torch.empty((b * P, D), dtype=BF16, device=dev)
        dw_eff = torch.empty((D, kcols), dtype=F32, device=dev)
        dconv = torch.empty(conv_shape, dtype=F32, device=dev) if mean_ch else dw_eff.view(conv_shape)
        dcls = torch.empty((D,), dtype=F32, device=dev)
        dpos = torch.empty(pos_shape, dtype=F32, device=dev)      # rows 0 .. P are written by the kernel
        if pos_shape[0] > P + 1:
            dpos[P + 1:].zero_()                                  # a table longer than the sequence: the unused rows' gradient
        dlnw = torch.empty((D,), dtype=F32, device=dev)
        dlnb = torch.empty((D,), dtype=F32, device=dev)
        ws = scratch("patch_embed_bwd", query("vipant_patch_embed_ln_bwd_workspace_bytes", b, P, D, kcols), dev)
        call("vipant_patch_embed_ln_bwd", dout.data_ptr(), int(dout_bf16), tok.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
             ln_w.detach().data_ptr(), patches.data_ptr(), dtok.data_ptr(), dpatch.data_ptr(), dw_eff.data_ptr(),
             dconv.data_ptr(), dcls.data_ptr(), dpos.data_ptr(), dlnw.data_ptr(), dlnb.data_ptr(), b, P, D, Cw, khw,
             int(mean_ch), ws.data_ptr(), ws.numel(), _stream())
        return None, dconv, dcls, dpos, dlnw, dlnb, None


# ---------------------------------------------------------------------------------- transformer
class _LayerGrads:
    """fp32 gradients of one block, carved from one flat buffer so a replica group can all-reduce a whole
    layer with a single RCCL call as soon as its backward is done."""

    def __init__(self, shapes: Sequence[torch.Size], device):
        sizes = [int(torch.Size(s).numel()) for s in shapes]
        pad = [(n + 3) // 4 * 4 for n in sizes]            # keep every view 16-byte aligned
        self.flat = torch.empty((sum(pad),), dtype=F32, device=device)
        self.views, off = [], 0
        for s, n, p in zip(shapes, sizes, pad):
            self.views.append(self.flat[off:off + n].view(s))
            off += p

    def publish(self, grads: list, l: int, params, grad_sync):
        """Hand block l's gradients to `grads` (12 per block, in parameter order) and start their all-reduce, if any."""
        grads[12 * l:12 * l + 12] = self.views
        if grad_sync is not None:
            grad_sync.reduce_async(self.flat, self.views, params[12 * l:12 * l + 12])


# precision of the residual-stream GRADIENT: `running.grad_stream` (bf16 | fp32; monitor.py sets it), default from the environment
GRAD_STREAM_F32 = os.environ.get("VIPANT_GRAD_STREAM", "bf16") == "fp32"
# the last block's one-query attention with the key / value projection folded into the query side (csrc/readout_ctx.hip);
# 0: project every token to K and V and attend over those (csrc/readout_rows.hip, the round-3 form)
LAST_BLOCK_CTX = os.environ.get("VIPANT_LAST_BLOCK_CTX", "1") != "0"
# 0: the e4m3 forms of the attention output and of dqkv by the stand-alone pass instead of the attention kernels' epilogues (A/B)
ATTN_EMIT = os.environ.get("VIPANT_ATTN_EMIT", "1") != "0"


def heads_to_wide(rows: torch.Tensor, w_t_cols: torch.Tensor, out: torch.Tensor, H: int) -> torch.Tensor:
    """out[(i, h), :] = rows[i, 64 h : 64 h + 64] . W_h, all heads in one launch (vipant_gemm_nt_heads): rows bf16 [n, D]; w_t_cols:
    the column block [:, c0 : c0 + D] of a TRANSPOSED weight matrix (bf16 [D, ld], a view: W_h^T is its columns 64 h ..); out bf16
    [n * H, D], or [2, n * H, D]: the result as a bf16 pair (hi plane, lo plane)."""
    n, D = rows.shape
    pair = out.dim() == 3
    assert D == 64 * H and tuple(out.shape[-2:]) == (n * H, D) and w_t_cols.shape == (D, D) and w_t_cols.stride(1) == 1 and out.is_contiguous()
    call("vipant_gemm_nt_heads", rows.data_ptr(), D, 64, 0, w_t_cols.data_ptr(), w_t_cols.stride(0), 64, out.data_ptr(), H * D, D,
         n * H * D if pair else 0, None, 0, n, D, 64, H, _stream())
    return out


def wide_to_heads(wide: torch.Tensor, w_rows: torch.Tensor, H: int, bias=None) -> torch.Tensor:
    """out[i, 64 h : 64 h + 64] = wide[(i, h), :] . W_h^T (+ bias of those columns), all heads in one launch: wide bf16 [n * H, D]
    (or a bf16 pair [2, n * H, D]: both planes enter the product); w_rows: the row block [r0 : r0 + D] of a weight matrix (bf16
    [D, D], contiguous: W_h is its rows 64 h ..); out bf16 [n, D]."""
    pair = wide.dim() == 3
    nH, D = wide.shape[-2:]
    n = nH // H
    assert D == 64 * H and nH % H == 0 and wide.is_contiguous() and w_rows.shape == (D, D) and w_rows.is_contiguous()
    out = torch.empty((n, D), dtype=BF16, device=wide.device)
    call("vipant_gemm_nt_heads", wide.data_ptr(), H * D, D, nH * D if pair else 0, w_rows.data_ptr(), D, 64 * D, out.data_ptr(), D, 64, 0,
         _ptr(bias), 64, n, 64, D, H, _stream())
    return out


def head_expand(rows: torch.Tensor, H: int) -> torch.Tensor:
    """rows bf16 [n, 64 H] -> [n * H, 64 H]: row (i, h) keeps head h's 64 columns of row i, zeros elsewhere."""
    _need(rows, BF16, "head_expand.rows")
    n, D = rows.shape
    assert D == 64 * H and rows.is_contiguous()
    out = torch.empty((n * H, D), dtype=BF16, device=rows.device)
    call("vipant_head_expand", rows.data_ptr(), out.data_ptr(), n, H, _stream())
    return out


def head_extract(full: torch.Tensor, H: int, bias=None) -> torch.Tensor:
    """full bf16 | fp32 [n * H, 64 H] -> bf16 [n, 64 H]: head h's 64 columns of row (i, h) (+ bias)."""
    nH, D = full.shape
    assert D == 64 * H and nH % H == 0 and full.is_contiguous() and full.dtype in (BF16, F32)
    out = torch.empty((nH // H, D), dtype=BF16, device=full.device)
    call("vipant_head_extract", full.data_ptr(), int(full.dtype == F32), _ptr(bias), out.data_ptr(), nH // H, H, _stream())
    return out


class _Stack:
    """Shapes and switches of one BackboneFn call, read by its forward, its backward (ctx.stack) and every block."""

    def __init__(self, device, batch, S, D, causal, train, fp8, recompute_mlp, stream_f16, ridx, prune):
        self.dev, self.batch, self.S, self.M, self.D, self.H = device, batch, S, batch * S, D, D // 64
        self.causal, self.train, self.fp8, self.recompute_mlp = bool(causal), train, bool(fp8), bool(recompute_mlp)
        self.ridx, self.prune, self.keep_mlp = ridx, prune, train and not recompute_mlp
        self.keep_q = self.fp8 and train and FP8_TN and D % 128 == 0    # the forward keeps e4m3 forms for the e4m3 weight-gradient contractions
        self.tn8 = FP8_TN        # (decided by the forward: the backward must read what that forward kept)
        self.ctx_alg = prune and LAST_BLOCK_CTX and self.H in (8, 12, 16) and S <= 1024
        # `running.stream_dtype: fp16`: inside the stack the residual stream is kept in the reference's own autocast precision
        # (clip/model.py:157-160) -- every LayerNorm pass reads and writes 2 instead of 4 bytes per element of it, and so do the
        # saved copies the backward reads; statistics stay fp32, the norm is taken on the unrounded sum, and the tensors that
        # cross the autograd boundary (the stack's input and output) stay fp32
        self.sdt = F16 if stream_f16 else F32

    def sflags(self, t):
        return (_ffi.STREAM_IN_F16 if t.dtype == F16 else 0) | (_ffi.STREAM_OUT_F16 if self.sdt == F16 else 0)

    def new(self, cols, dtype=BF16, rows=None):
        return torch.empty((self.M if rows is None else rows, cols), dtype=dtype, device=self.dev)


class _Record:
    """A block's state between its forward and its backward, by name; a field the forward did not set is None."""
    __slots__ = ()

    def __init__(self, **fields):
        for k in self.__slots__:
            setattr(self, k, fields.pop(k, None))
        assert not fields, fields


class _Block(_Record):
    """What a full block's backward reads: activations (an e4m3 form as ONE (bytes, block scales) pair: h1q, h2q, oq, gq), W^T of
    in_proj, out_proj, c_fc, c_proj (bf16 wt, e4m3 wtq) and c_fc's W (bf16 wfc_b, e4m3 q_fc) for the MLP recomputation."""
    __slots__ = ("x", "mean1", "rstd1", "h1", "h1q", "qkv", "o", "oq", "lse", "x1", "mean2", "rstd2", "h2", "h2q", "u", "g", "gq",
                 "wt", "wtq", "wfc_b", "q_fc")


class _RowsBlock(_Record):
    """What the backward of the last block on the read-out rows reads (*_r: `batch` rows; wqkv_b: in_proj W of the folded form)."""
    __slots__ = ("x", "mean1", "rstd1", "h1", "qkv", "q_r", "probs", "o_r", "h1_r", "x1_r", "mean2_r", "rstd2_r", "h2_r", "u_r", "g_r",
                 "wt", "wqkv_b")


def _block_fwd(s: _Stack, b: _Block, x, y_prev, p, wb, wq, tmp):
    """One full block forward; `b` receives the activations (buffers of its own when training, the shared temporaries `tmp` of a
    frozen tower).  Returns (x1, y2): the stream after the attention half and the MLP branch's output, added by the next LayerNorm."""
    M, D, H, new, fp8, st = s.M, s.D, s.H, s.new, s.fp8, _stream()
    ln1w, ln1b, _, bqkv, _, bo, ln2w, ln2b, _, bfc, _, bpr = p
    (wqkv_b, wo_b, wfc_b, wpr_b), (q_qkv, q_o, q_fc, q_pr) = wb, wq or (None,) * 4
    emit_o = fp8 and H % 2 == 0 and ATTN_EMIT     # the attention kernel leaves its output's e4m3 form, what out_proj reads
    if not s.train:
        b.h1, b.h2, b.qkv, y1, y2 = tmp.h1, tmp.h2, tmp.qkv, tmp.y1, tmp.y2
        b.mean1, b.rstd1 = b.mean2, b.rstd2 = tmp.stats
    else:
        b.qkv, y1, y2 = new(3 * D), new(D), new(D)
        (b.mean1, b.rstd1), (b.mean2, b.rstd2) = _stats(M, s.dev), _stats(M, s.dev)
        if s.keep_q:
            # e4m3 weight gradients: of the two LayerNorm outputs and of g the backward reads the e4m3 forms alone (block-uniform
            # scales: static ones from the LayerNorm passes, the c_fc epilogue's for g) -- 1 instead of 2 bytes per element kept, and
            # the bf16 tensors are never written; the attention output's e4m3 form (what out_proj reads) is kept beside the bf16 one
            # the attention backward needs
            b.oq = mx_buffer(M, D, s.dev) if emit_o else None
            b.h1q, b.h2q = mx_buffer(M, D, s.dev), mx_buffer(M, D, s.dev)
        else:
            b.h1, b.h2 = new(D), new(D)
            # `recompute_mlp` under e4m3: the LayerNorm output's e4m3 form is kept beside it (M D bytes + scales per block), so
            # that the backward's c_fc launch needs no quantisation pass either
            b.h2q = mx_buffer(M, D, s.dev) if (fp8 and s.recompute_mlp) else None
        if s.keep_mlp:      # u: 8-bit codes of QuickGELU'(pre-activation) -- all the backward needs of it
            b.u = new(4 * D, torch.uint8)
            b.gq, b.g = (mx_buffer(M, 4 * D, s.dev), None) if s.keep_q else (None, new(4 * D))
    u, g = (b.u, b.g) if s.keep_mlp else (tmp.u, tmp.g)
    # ln_1 (+ residual add of the previous block's MLP branch: x <- x + y2_prev) + in_proj
    xs = new(D, s.sdt) if y_prev is not None else None
    call("vipant_ln_qkv_fwd", x.data_ptr(), _ptr(y_prev), _ptr(xs), ln1w.data_ptr(), ln1b.data_ptr(), wqkv_b.data_ptr(),
         bqkv.data_ptr(), _ptr(b.h1), b.mean1.data_ptr(), b.rstd1.data_ptr(), b.qkv.data_ptr(), M, D,
         C.byref(fp8_plan(q_qkv, None, b.h1q or tmp.act)) if fp8 else None, s.sflags(x), st)
    b.x = x = xs if xs is not None else x
    q8 = (b.oq or tmp.act) if emit_o else None
    b.o, b.lse = mha_fwd(b.qkv, s.batch, s.S, H, s.causal, q8=q8)
    call("vipant_gemm_bias_residual_fwd", None if q8 else b.o.data_ptr(), wo_b.data_ptr(), bo.data_ptr(), None, y1.data_ptr(),
         M, D, D, C.byref(fp8_plan(q_o, None, q8 or tmp.act)) if fp8 else None, st)
    # ln_2 (+ residual add of the attention branch) + c_fc + QuickGELU + c_proj
    b.x1 = new(D, s.sdt)
    if "gemm_nt" in KERNEL_PROBE and not fp8:     # bench.py times the c_fc launch alone: the same three launches, issued one by one
        call("vipant_layernorm_fwd", x.data_ptr(), D, ln2w.data_ptr(), ln2b.data_ptr(), b.h2.data_ptr(), None,
             b.mean2.data_ptr(), b.rstd2.data_ptr(), M, D, y1.data_ptr(), b.x1.data_ptr(), None, None, s.sflags(x), st)
        gemm_nt(b.h2, wfc_b, g, bias=bfc, aux=u, epi=EPI_QUICKGELU_D8)
        gemm_nt(g, wpr_b, y2, bias=bpr, epi=EPI_BF16)
    else:
        only_q = fp8 and not s.keep_mlp        # c_proj's operand is all that is wanted of g: neither g nor the codes are written
        call("vipant_ln_mlp_quickgelu_fwd", x.data_ptr(), y1.data_ptr(), b.x1.data_ptr(), ln2w.data_ptr(), ln2b.data_ptr(),
             wfc_b.data_ptr(), bfc.data_ptr(), wpr_b.data_ptr(), bpr.data_ptr(), _ptr(b.h2), b.mean2.data_ptr(),
             b.rstd2.data_ptr(), None if only_q else u.data_ptr(), None if (only_q or g is None) else g.data_ptr(), y2.data_ptr(), M, D,
             C.byref(fp8_plan(q_fc, q_pr, b.h2q or tmp.act, emit=b.gq or tmp.emit)) if fp8 else None, s.sflags(x), st)
    return b.x1, y2


def _rows_block_fwd(s: _Stack, b: _RowsBlock, x, y_prev, p, wb, tmp):
    """The last block on the read-out rows: bf16 contractions whatever `fp8` says -- all of them launches on `batch` or `batch * H`
    rows.  (Only the round-3 form, VIPANT_LAST_BLOCK_CTX=0, still has a per-token launch here, the K / V projection, N = 2 D: it
    stays bf16 too, a documented departure from `running.fp8_gemm` for 1 of 97 contraction launches.)  `running.last_block_rows=False`
    restores the e4m3 last block; both corners are under test_end_to_end_golden_e4m3.  Returns the rows' output, fp32 [batch, D]."""
    M, D, H, batch, S, ridx, new, dev, st = s.M, s.D, s.H, s.batch, s.S, s.ridx, s.new, s.dev, _stream()
    ln1w, ln1b, wqkv, bqkv, _, bo, ln2w, ln2b, _, bfc, _, bpr = p
    wqkv_b, wo_b, wfc_b, wpr_b = wb
    # (training: the last block keeps its per-token activations for the read-out rows only)
    b.h1, (b.mean1, b.rstd1) = (new(D), _stats(M, dev)) if s.train else (tmp.h1, tmp.stats)
    xs = new(D, s.sdt) if y_prev is not None else None
    call("vipant_layernorm_fwd", x.data_ptr(), D, ln1w.data_ptr(), ln1b.data_ptr(), b.h1.data_ptr(), None,
         b.mean1.data_ptr(), b.rstd1.data_ptr(), M, D, _ptr(y_prev), _ptr(xs), None, None, s.sflags(x), st)
    b.x = x = xs if xs is not None else x
    b.h1_r = gather_rows(b.h1, ridx, batch, S)
    b.q_r = gemm_nt(b.h1_r, wqkv_b[:D], new(D, rows=batch), bias=bqkv[:D], epi=EPI_BF16, few_rows=True)     # Q of the read-out rows
    b.probs = torch.empty((batch, H, S), dtype=F32, device=dev)
    if s.ctx_alg:
        # one query per (item, head): the key projection moves to the query (qk_h = W_k,h^T q_h, the key bias drops out of the
        # softmax), the value projection behind the weighted sum (o_h = W_v,h sum_j p_j h1_j + b_v,h): two per-head contractions on
        # `batch` rows and one pass over h1 instead of K, V of every token
        wk_t = (b.wt[0] if s.train else cached_bf16(wqkv, transpose_only=True))[:, D:2 * D]
        # qk and the heads' contexts travel as bf16 PAIRS (hi + lo planes, round 5): [0]: qk, [1]: contexts
        b.qkv = torch.empty((2, 2, batch * H, D), dtype=BF16, device=dev)
        heads_to_wide(b.q_r, wk_t, b.qkv[0], H)
        call("vipant_rows_ctx_fwd", b.qkv[0].data_ptr(), b.h1.data_ptr(), _ptr(ridx), b.qkv[1].data_ptr(), b.probs.data_ptr(),
             batch, S, H, int(s.causal), 1, st)
        b.o_r = wide_to_heads(b.qkv[1], wqkv_b[2 * D:], H, bias=bqkv[2 * D:])
    else:
        b.qkv = new(3 * D) if s.train else tmp.qkv
        gemm_nt(b.h1, wqkv_b[D:], b.qkv[:, D:], bias=bqkv[D:], epi=EPI_BF16)         # K, V of every token
        b.o_r = new(D, rows=batch)
        call("vipant_mha_rows_fwd", b.q_r.data_ptr(), b.qkv.data_ptr(), _ptr(ridx), b.o_r.data_ptr(), b.probs.data_ptr(), batch, S,
             H, int(s.causal), st)
    y1_r = gemm_nt(b.o_r, wo_b, new(D, rows=batch), bias=bo, epi=EPI_BF16, few_rows=True)
    x_r = gather_rows(x, ridx, batch, S)
    # the read-out rows' stream stays fp32 from here, and c_proj adds it in its epilogue: the rows the features are read from skip
    # the two roundings (fp16 stream, bf16 branch output) the full block would give them
    b.x1_r, b.h2_r, b.u_r, b.g_r = new(D, F32, batch), new(D, rows=batch), new(4 * D, torch.uint8, batch), new(4 * D, rows=batch)
    b.mean2_r, b.rstd2_r = _stats(batch, dev)
    call("vipant_layernorm_fwd", x_r.data_ptr(), D, ln2w.data_ptr(), ln2b.data_ptr(), b.h2_r.data_ptr(), None,
         b.mean2_r.data_ptr(), b.rstd2_r.data_ptr(), batch, D, y1_r.data_ptr(), b.x1_r.data_ptr(), None, None,
         _ffi.STREAM_IN_F16 if x_r.dtype == F16 else 0, st)
    gemm_nt(b.h2_r, wfc_b, b.g_r, bias=bfc, aux=b.u_r, epi=EPI_QUICKGELU_D8, few_rows=True)
    return gemm_nt(b.g_r, wpr_b, new(D, F32, batch), bias=bpr, aux=b.x1_r, epi=EPI_RESIDUAL_F32, few_rows=True)


def _block_bwd(s: _Stack, b: _Block, p, lg: _LayerGrads, lg_below: Optional[_LayerGrads], dx, dx_b, dyq, tmp):
    """One full block backward, in place on the stream gradient: dx (fp32 master | None), dx_b (bf16), dyq (its e4m3 form | None).
    The block's parameter gradients go to `lg`, d c_proj.bias of the block below to `lg_below`."""
    M, D, H, fp8, kq, ws, st = s.M, s.D, s.H, s.fp8, s.keep_q, tmp.ws, _stream()
    ln1w, _, _, _, _, _, ln2w, _, _, bfc, _, _ = p
    (wqkv_t, wo_t, wfc_t, wpr_t), (tq_qkv, tq_o, tq_fc, tq_pr) = b.wt, b.wtq or (None,) * 4
    d_ln1w, d_ln1b, d_wqkv, d_bqkv, d_wo, d_bo, d_ln2w, d_ln2b, d_wfc, d_bfc, d_wpr, d_bpr = lg.views
    if s.recompute_mlp:
        # (e4m3 weight gradients: the recomputation leaves g's e4m3 form -- the same epilogue, the same bytes as a forward that keeps
        # it -- and no bf16 g)
        u, g, keep = tmp.u, tmp.g, tmp.gq
        call("vipant_mlp_quickgelu_recompute", None if fp8 else b.h2.data_ptr(), b.wfc_b.data_ptr(), bfc.data_ptr(), u.data_ptr(),
             None if kq else g.data_ptr(), M, D, C.byref(fp8_plan(b.q_fc, None, b.h2q, emit=keep)) if fp8 else None, st)
        if not kq:
            b.h2q = None        # read by the recomputation alone
    else:
        u, g, keep = b.u, b.g, b.gq
    keep1, keep2 = (b.h1q, b.h2q) if kq else (None, None)     # h1, h2 (and g) as the e4m3 forms the forward kept
    # MLP half: c_proj^T + QuickGELU', c_fc^T, both weight gradients, ln_2 backward (+ residual gradient);
    # the produced stream gradient is also d(out_proj output): its column sum is d out_proj.bias
    call("vipant_ln_mlp_quickgelu_bwd", dx_b.data_ptr(), wpr_t.data_ptr(), wfc_t.data_ptr(), u.data_ptr(),
         None if keep else g.data_ptr(), None if keep2 else b.h2.data_ptr(), b.x1.data_ptr(), b.mean2.data_ptr(), b.rstd2.data_ptr(),
         ln2w.data_ptr(), _ptr(dx), dx_b.data_ptr(), _ptr(tmp.du), tmp.dh.data_ptr(), d_wpr.data_ptr(), d_wfc.data_ptr(),
         d_bfc.data_ptr(), d_ln2w.data_ptr(), d_ln2b.data_ptr(), d_bo.data_ptr(), M, D, ws.data_ptr(), ws.numel(),
         C.byref(fp8_plan(tq_pr, tq_fc, tmp.act, dyq, emit=tmp.emit, tn=s.tn8, keep=keep, keep2=keep2)) if fp8 else None,
         _ffi.STREAM_IN_F16 if b.x1.dtype == F16 else 0, st)
    # attention half: out_proj^T, attention core, in_proj^T + ln_1 backward; the produced stream gradient is
    # d(c_proj output) of the block below: its column sum is that block's d c_proj.bias
    call("vipant_gemm_bias_residual_bwd", dx_b.data_ptr(), wo_t.data_ptr(), b.o.data_ptr(), tmp.do.data_ptr(), d_wo.data_ptr(),
         M, D, D, ws.data_ptr(), ws.numel(),
         C.byref(fp8_plan(tq_o, None, tmp.act, dyq, emit=tmp.emit, tn=s.tn8, keep=b.oq)) if fp8 else None, st)
    q8 = tmp.act if (fp8 and H % 2 == 0 and ATTN_EMIT) else None
    dqkv = mha_bwd(b.qkv, b.o, tmp.do, b.lse, s.batch, s.S, H, s.causal, q8=q8)
    call("vipant_ln_qkv_bwd", dqkv.data_ptr(), wqkv_t.data_ptr(), None if keep1 else b.h1.data_ptr(), b.x.data_ptr(),
         b.mean1.data_ptr(), b.rstd1.data_ptr(), ln1w.data_ptr(), _ptr(dx), dx_b.data_ptr(), tmp.dh.data_ptr(), d_wqkv.data_ptr(),
         d_bqkv.data_ptr(), d_ln1w.data_ptr(), d_ln1b.data_ptr(), lg_below.views[11].data_ptr() if lg_below is not None else None,
         M, D, ws.data_ptr(), ws.numel(), C.byref(fp8_plan(tq_qkv, None, tmp.act, dyq, emit=tmp.emit, tn=s.tn8, keep=keep1)) if fp8 else None,
         (_ffi.STREAM_IN_F16 if b.x.dtype == F16 else 0) | (_ffi.STREAM_ACT_Q if q8 else 0), st)


def _rows_block_bwd(s: _Stack, b: _RowsBlock, p, lg: _LayerGrads, lg_below: Optional[_LayerGrads], dxr_b, tmp):
    """The last block on the read-out rows, backward from dxr_b (bf16 [batch, D]): the two block operators of the MLP / out_proj half
    on `batch` rows, the one-query attention backward, then the K / V half of in_proj and ln_1 on every token.  Returns the stream
    gradient below it, (dx, dx_b, dyq)."""
    M, D, H, batch, S, ridx, dev, ws, dh, st = s.M, s.D, s.H, s.batch, s.S, s.ridx, s.dev, tmp.ws, tmp.dh, _stream()
    ln1w, _, _, _, _, _, ln2w, _, _, _, _, _ = p
    wqkv_t, wo_t, wfc_t, wpr_t = b.wt
    d_ln1w, d_ln1b, d_wqkv, d_bqkv, d_wo, d_bo, d_ln2w, d_ln2b, d_wfc, d_bfc, d_wpr, d_bpr = lg.views
    du_r, dh_r, do_r = s.new(4 * D, rows=batch), s.new(D, rows=batch), s.new(D, rows=batch)
    call("vipant_ln_mlp_quickgelu_bwd", dxr_b.data_ptr(), wpr_t.data_ptr(), wfc_t.data_ptr(), b.u_r.data_ptr(),
         b.g_r.data_ptr(), b.h2_r.data_ptr(), b.x1_r.data_ptr(), b.mean2_r.data_ptr(), b.rstd2_r.data_ptr(), ln2w.data_ptr(), None,
         dxr_b.data_ptr(), du_r.data_ptr(), dh_r.data_ptr(), d_wpr.data_ptr(), d_wfc.data_ptr(), d_bfc.data_ptr(),
         d_ln2w.data_ptr(), d_ln2b.data_ptr(), d_bo.data_ptr(), batch, D, ws.data_ptr(), ws.numel(), None,
         (_ffi.STREAM_IN_F16 if b.x1_r.dtype == F16 else 0) | _ffi.STREAM_FEW_ROWS, st)
    # out_proj backward on the rows (vipant_gemm_bias_residual_bwd's two launches, the first as a few-rows launch)
    gemm_nt(dxr_b, wo_t, do_r, epi=EPI_BF16, few_rows=True)
    gemm_tn(dxr_b, b.o_r, d_wo, ws_name="block_bwd")
    if s.ctx_alg:
        # qkv = [qk | contexts] of the forward.  dctx_h = W_v,h^T do_h; the kernel gives dh of every token and dqk;
        # dq_h = W_k,h dqk_h; d W_v = do (x) ctx, d W_k = q (x) dqk per head (block-sparse operands), d b_k = 0
        # (qk, the contexts and dqk are bf16 pairs; the two weight gradients take the hi planes: their own rounding, fp32
        # sums over `batch * H` bf16 products, is the larger term)
        qk, hctx = b.qkv[0], b.qkv[1]
        dctx = heads_to_wide(do_r, wqkv_t[:, 2 * D:], torch.empty((batch * H, D), dtype=BF16, device=dev), H)
        gemm_tn(head_expand(do_r, H), hctx[0], d_wqkv[2 * D:], a_colsum=d_bqkv[2 * D:], ws_name="block_bwd")
        dqk = torch.empty((2, batch * H, D), dtype=BF16, device=dev)
        call("vipant_rows_ctx_bwd", qk.data_ptr(), dctx.data_ptr(), hctx.data_ptr(), b.h1.data_ptr(), _ptr(ridx),
             b.probs.data_ptr(), dh.data_ptr(), dqk.data_ptr(), d_bqkv[D:2 * D].data_ptr(), batch, S, H, int(s.causal), 1, st)
        dq_r = wide_to_heads(dqk, b.wqkv_b[D:2 * D], H)
        gemm_tn(head_expand(b.q_r, H), dqk[0], d_wqkv[D:2 * D], ws_name="block_bwd")
        del dctx, dqk
    else:
        dq_r, dqkv = s.new(D, rows=batch), s.new(3 * D)
        call("vipant_mha_rows_bwd", b.q_r.data_ptr(), b.qkv.data_ptr(), _ptr(ridx), b.probs.data_ptr(), do_r.data_ptr(),
             dq_r.data_ptr(), dqkv.data_ptr(), batch, S, H, int(s.causal), st)
        # dh = dK|dV . W_kv on every token
        gemm_nt(dqkv[:, D:], wqkv_t[:, D:], dh, epi=EPI_BF16)
        gemm_tn(dqkv[:, D:], b.h1, d_wqkv[D:], a_colsum=d_bqkv[D:], ws_name="block_bwd")
        del dqkv
    # + dq . W_q on the read-out rows
    dhq = gemm_nt(dq_r, wqkv_t[:, :D], torch.empty((batch, D), dtype=F32, device=dev), epi=EPI_F32, few_rows=True)
    call("vipant_add_rows_bf16", dh.data_ptr(), _ptr(ridx), dhq.data_ptr(), 1, batch, S, D, st)
    gemm_tn(dq_r, b.h1_r, d_wqkv[:D], a_colsum=d_bqkv[:D], ws_name="block_bwd")
    # ln_1 backward on every token; the residual gradient of this block exists on the read-out rows only
    dx_b = torch.empty((M, D), dtype=BF16, device=dev)
    call("vipant_layernorm_bwd", dh.data_ptr(), _ffi.LN_X_F16 if b.x.dtype == F16 else 0, b.x.data_ptr(), D,
         b.mean1.data_ptr(), b.rstd1.data_ptr(), ln1w.data_ptr(), None, None, D, dx_b.data_ptr(), d_ln1w.data_ptr(),
         d_ln1b.data_ptr(), lg_below.views[11].data_ptr() if lg_below is not None else None, 0, M, D, ws.data_ptr(),
         ws.numel(), None, None, st)
    call("vipant_add_rows_bf16", dx_b.data_ptr(), _ptr(ridx), dxr_b.data_ptr(), 0, batch, S, D, st)
    if lg_below is not None:
        colsum(dxr_b, lg_below.views[11], accumulate=True)
    dx = s.new(D, F32) if GRAD_STREAM_F32 else None
    if dx is not None:
        call("vipant_cast_f32", dx_b.data_ptr(), dx.data_ptr(), M * D, st)
    return dx, dx_b, (quant_e4m3_mx(dx_b) if s.fp8 else None)


class BackboneFn(torch.autograd.Function):
    """TransformerBackbone.forward = L x ResidualAttentionBlock (cvap/module/val.py:493-522) on the fp32
    residual stream x [batch*S, D].  One autograd node for the whole stack: the layer loop, the saved
    activations and the (fp32, bf16) gradient-stream pair between layers are managed here, not by autograd.
    Per block four entry points of the fused operator set each way (include/vipant_hip.h): vipant_ln_qkv_*, vipant_mha_*,
    vipant_gemm_bias_residual_*, vipant_ln_mlp_quickgelu_*.  Each block runs through _block_fwd / _block_bwd; what its backward
    reads of its forward is one named record per block (_Block), kept on ctx and dropped as soon as that block's backward is done.

    `rows` (None | "first" | int64 [batch]): the caller will read ONE row per item of the output -- the class token
    (ViTPostEncoder, cvap/module/val.py:288-289) or the end-of-text token (GPTPostEncoder, val.py:143-145) -- and the node returns
    just those rows, [batch, D].  The last block is then evaluated on them alone (_rows_block_fwd / _rows_block_bwd, record
    _RowsBlock; csrc/readout_rows.hip): ln_1 and the key / value projection see every token, the query projection, the attention
    (one query per item and head), out_proj, ln_2 and the MLP see `batch` rows, forward and backward.  Exact: the other rows of the
    last block's output are never read and carry no gradient, so every feature and every parameter gradient is what the full block
    gives (tests/test_model_gpu.py, against the reference's vectors and against rows=None)."""

    @staticmethod
    def forward(ctx, x_in, batch, S, causal, grad_sync, recompute_mlp, fp8, stream_f16, rows, *params):
        _need(x_in, F32, "backbone.x")
        (M, D), L = x_in.shape, len(params) // 12
        assert M == batch * S and len(params) % 12 == 0
        ridx = rows if isinstance(rows, torch.Tensor) else None
        if ridx is not None:
            _need(ridx, I64, "backbone.rows")
            assert ridx.numel() == batch and ridx.is_contiguous()
        x = x0 = x_in.contiguous()
        s = _Stack(x.device, batch, S, D, causal, any(ctx.needs_input_grad), fp8, recompute_mlp, stream_f16, ridx,
                   rows is not None and L > 0)
        # Per block (cvap/module/val.py:519-522):  x1 = x + attn(ln_1(x));  x2 = x1 + mlp(ln_2(x1)).
        # The branch outputs y1, y2 leave their contraction as bf16 and the residual add is fused into the NEXT
        # LayerNorm pass (fp32 stream in, fp32 stream + bf16 normalised activations out), so every contraction has a
        # plain single-output bf16 epilogue and the fp32 stream is only touched by the streaming LN kernels.
        tmp = SimpleNamespace(u=None, g=None, act=None, emit=None)      # temporaries every block shares
        if not s.train:     # frozen tower: one set of temporaries for all layers
            tmp.h1, tmp.h2, tmp.qkv, tmp.y1, tmp.y2, tmp.stats = s.new(D), s.new(D), s.new(3 * D), s.new(D), s.new(D), _stats(M, s.dev)
        # (e4m3 towers that do not keep the MLP activations need neither: the c_fc epilogue leaves g's e4m3 form for c_proj and nothing else)
        if not s.keep_mlp and not s.fp8:
            tmp.u, tmp.g = s.new(4 * D, torch.uint8), s.new(4 * D)
        # e4m3 operands in the NT contractions (configs[4]): a property of the tower, whether or not this call records a backward --
        # the no-grad feature pass of `running.micro_batch` and evaluation must see the forward the training pass differentiates
        if s.train or s.fp8:        # bf16 copies (W and W^T) of the 4 L weight matrices: one launch per step
            mats = [params[12 * l + i] for l in range(L) for i in (2, 4, 8, 10)]
            wb_all, wt_all, wq_all, wtq_all = cast_weights(mats, e4m3=True) if s.fp8 else (*cast_weights(mats), None, None)
            if s.fp8:
                tmp.act, tmp.emit = fp8_scratch(M, D, s.dev), fp8_scratch(M, D, s.dev)
        blocks, y_prev = [], None
        for l in range(L):
            p = [t.detach() for t in params[12 * l:12 * l + 12]]
            mine = slice(4 * l, 4 * l + 4)          # this block's in_proj, out_proj, c_fc, c_proj in the weight lists
            wb = wb_all[mine] if (s.train or s.fp8) else [cached_bf16(p[i]) for i in (2, 4, 8, 10)]
            wq = wq_all[mine] if s.fp8 else None
            wt, wtq = (wt_all[mine], wtq_all[mine] if s.fp8 else None) if s.train else (None, None)
            if s.prune and l == L - 1:
                b = _RowsBlock(wt=wt, wqkv_b=wb[0] if s.ctx_alg else None)
                x, y_prev = _rows_block_fwd(s, b, x, y_prev, p, wb, tmp), None
            else:
                b = _Block(wt=wt, wtq=wtq, wfc_b=wb[2] if s.recompute_mlp else None, q_fc=wq[2] if s.fp8 and s.recompute_mlp else None)
                x, y_prev = _block_fwd(s, b, x, y_prev, p, wb, wq, tmp)
            if s.train:
                blocks.append(b)
        x = residual_add(x, y_prev) if y_prev is not None else x
        if s.train:
            # the stack's input (version-checked by autograd) and parameters go through autograd; the blocks' own state is the records
            ctx.save_for_backward(x0, *params)
            ctx.stack, ctx.blocks, ctx.grad_sync = s, blocks, grad_sync
            ctx._vipant_kind = "stack"
            ctx.readout_grad = None                      # (idx | None, compact fp32 rows), handed over by ReadoutFn.backward
            ctx.patch_node = _producer(x_in, "patch")    # the patch embedding that produced this stack's input, if any
        return x

    @staticmethod
    def backward(ctx, dx_in):
        if ctx.blocks is None:
            raise _ffi.VipantError("BackboneFn: second backward through the same forward -- the node releases its bf16 weight copies "
                                   "and saved activations in its first backward (retain_graph re-entry is not supported)")
        s, blocks, ctx.blocks = ctx.stack, ctx.blocks, None
        _, *params = ctx.saved_tensors
        L, M, D, S, dev = len(params) // 12, s.M, s.D, s.S, s.dev
        # Gradient of the residual stream.  Default: bf16 only -- the tensor the next contraction reads IS the stream (LayerNorm
        # backward 10 instead of 16 B per element); the forward stream stays fp32, so the loss and the features are untouched and
        # the gradients move from ~1.3 % to ~1.6 % rel-L2 of the fp32 reference (profiles/r2_stream_precision.md, model D; the
        # reference's own GPU path keeps this stream in fp16).  VIPANT_GRAD_STREAM=fp32: fp32 master + bf16 copy, both in place.
        handed, ctx.readout_grad = ctx.readout_grad, None
        dx = None
        if s.prune:
            # the gradient arrives for the read-out rows only, [batch, D]: dense, or handed over by the read-out node
            if handed is not None:
                dx_in = handed[1] if _is_placeholder(dx_in, handed[2]) else dx_in + handed[1]
            dx_b, top = None, cast_bf16_flat(dx_in.contiguous())
        elif handed is not None and _is_placeholder(dx_in, handed[2]) and not GRAD_STREAM_F32:
            # the read-out's gradient as compact rows: they go straight into a zeroed bf16 stream gradient
            idx, rows, _ = handed
            dx_b = torch.zeros((M, D), dtype=BF16, device=dev)
            top = torch.empty((rows.shape[0], D), dtype=BF16, device=dev)
            call("vipant_scatter_rows_bf16", rows.data_ptr(), _ptr(idx), dx_b.data_ptr(), top.data_ptr(), rows.shape[0], S, D, _stream())
        else:
            if handed is not None:                       # dense gradient from another consumer: add the read-out rows to it
                idx, rows, _ = handed
                dx_in = dx_in.contiguous().clone()
                call("vipant_scatter_rows", rows.data_ptr(), _ptr(idx), dx_in.data_ptr(), rows.shape[0], S, D, _stream())
            dx = dx_in.contiguous().clone() if GRAD_STREAM_F32 else None
            dx_b = top = cast_bf16_flat(dx if dx is not None else dx_in.contiguous())
        # scratch shared by all blocks (e4m3 weight gradients: du exists in its e4m3 form alone, in `emit`)
        tmp = SimpleNamespace(ws=scratch("block_bwd", query("vipant_block_workspace_bytes", M, D), dev), act=None, emit=None)
        if s.fp8:
            tmp.act, tmp.emit = fp8_scratch(M, D, dev), fp8_scratch(M, D, dev)
        # from here on every LayerNorm backward leaves the new stream gradient's e4m3 form beside it
        dyq = quant_e4m3_mx(dx_b) if (s.fp8 and not s.prune) else None
        tmp.du, tmp.dh, tmp.do = None if s.keep_q else s.new(4 * D), s.new(D), s.new(D)
        if s.recompute_mlp:
            tmp.u, tmp.g = s.new(4 * D, torch.uint8), None if s.keep_q else s.new(4 * D)
            tmp.gq = mx_buffer(M, 4 * D, dev) if s.keep_q else None
        grads: List[Optional[torch.Tensor]] = [None] * (12 * L)
        lg = _LayerGrads([p.shape for p in params[12 * (L - 1):12 * L]], dev)
        # d c_proj.bias of the top block (lower blocks get theirs from ln_1's backward): column sums of the stream gradient, which
        # with a handed-over read-out gradient has only those rows
        colsum(top, lg.views[11])
        for l in reversed(range(L)):
            p = [t.detach() for t in params[12 * l:12 * l + 12]]
            lg_below = _LayerGrads([t.shape for t in params[12 * (l - 1):12 * l]], dev) if l > 0 else None
            # (a record leaves `blocks` here: it is dropped when its block's backward returns)
            if s.prune and l == L - 1:
                dx, dx_b, dyq = _rows_block_bwd(s, blocks.pop(), p, lg, lg_below, top, tmp)
            else:
                _block_bwd(s, blocks.pop(), p, lg, lg_below, dx, dx_b, dyq, tmp)
            lg.publish(grads, l, params, ctx.grad_sync)
            lg = lg_below
        need = ctx.needs_input_grad
        patch = ctx.patch_node                      # kept: a second backward over a retained graph hands over again
        if dx is None and need[0]:
            if patch is not None:        # the patch embedding's LayerNorm backward takes the bf16 stream gradient as it is
                dx = _placeholder((M, D), dev)
                patch.stream_grad = (dx_b, dx)      # (whatever an earlier, never-consumed hand-off left there is replaced)
            else:
                dx = torch.empty((M, D), dtype=F32, device=dev)
                call("vipant_cast_f32", dx_b.data_ptr(), dx.data_ptr(), M * D, _stream())
        out_grads = [gr if need[9 + i] else None for i, gr in enumerate(grads)]
        return (dx if need[0] else None, None, None, None, None, None, None, None, None, *out_grads)


# ---------------------------------------------------------------------------------- read-out
class ReadoutFn(torch.autograd.Function):
    """ViTPostEncoder / GPTPostEncoder (cvap/module/val.py:288-289, 143-145) + the optional L2 normalisation of
    MetaHead.forward (clip_head.py:117-118): LN(x[b, idx_b]) @ proj -> [batch, E] fp32 -- vipant_cls_ln_proj_l2norm_{fwd,bwd}."""

    @staticmethod
    def forward(ctx, x, idx, batch, S, ln_w, ln_b, proj, normalized):
        _need(x, F32, "readout.x")
        x_arg = x
        x = x.contiguous()
        D, E = proj.shape
        dev = x.device
        train = any(ctx.needs_input_grad)
        rows = torch.empty((batch, D), dtype=F32, device=dev) if idx is not None else None
        y = torch.empty((batch, D), dtype=BF16, device=dev)
        mean, rstd = _stats(batch, dev)
        if train:
            proj_b, proj_t = cast_bf16(proj.detach(), True)
        else:
            proj_b, proj_t = None, cached_bf16(proj, transpose_only=True)
        feat = torch.empty((batch, E), dtype=F32, device=dev)
        out = torch.empty_like(feat) if normalized else feat
        norm = torch.empty((batch,), dtype=F32, device=dev) if normalized else None
        call("vipant_cls_ln_proj_l2norm_fwd", x.data_ptr(), _ptr(idx), ln_w.detach().data_ptr(), ln_b.detach().data_ptr(),
             proj_t.data_ptr(), _ptr(rows), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), feat.data_ptr(), out.data_ptr(), _ptr(norm),
             batch, S, D, E, int(bool(normalized)), _stream())
        if train:
            ctx.save_for_backward(x, idx, rows, y, mean, rstd, ln_w, proj_b, out, norm)
            ctx.meta = (batch, S, D, E, bool(normalized))
            ctx.stack_node = _producer(x_arg, "stack")       # the transformer stack whose output is read out, if any
        return out

    @staticmethod
    def backward(ctx, dout):
        x, idx, rows, y, mean, rstd, ln_w, proj_b, out, norm = ctx.saved_tensors
        batch, S, D, E, normalized = ctx.meta
        dev = dout.device
        dout = dout.contiguous()
        dfeat = torch.empty((batch, E), dtype=BF16, device=dev)
        dy = torch.empty((batch, D), dtype=BF16, device=dev)
        stack = ctx.stack_node                       # kept across backward calls (retain_graph)
        if stack is not None and stack.readout_grad is not None:
            stack.readout_grad = None                # left by a backward in which the stack's node never ran: not this call's business
        compact = stack is not None and ctx.needs_input_grad[0]
        drows = torch.empty((batch, D), dtype=F32, device=dev) if (idx is not None or compact) else None
        dproj = torch.empty((D, E), dtype=F32, device=dev)
        dlnw = torch.empty((D,), dtype=F32, device=dev)
        dlnb = torch.empty((D,), dtype=F32, device=dev)
        dx = None if compact else torch.zeros_like(x)
        ws = scratch("readout_bwd", query("vipant_cls_ln_proj_l2norm_bwd_workspace_bytes", batch, D, E), dev)
        call("vipant_cls_ln_proj_l2norm_bwd", dout.data_ptr(), out.data_ptr(), _ptr(norm), x.data_ptr(), _ptr(idx), _ptr(rows),
             y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ln_w.detach().data_ptr(), proj_b.data_ptr(), dfeat.data_ptr(),
             dy.data_ptr(), _ptr(drows), _ptr(dx), dproj.data_ptr(), dlnw.data_ptr(), dlnb.data_ptr(), batch, S, D, E,
             int(normalized), ws.data_ptr(), ws.numel(), _stream())
        if compact:                  # hand the rows to the stack's backward; autograd gets a zero-stride placeholder
            dx = _placeholder(tuple(x.shape), dev)
            stack.readout_grad = (idx, drows, dx)
        return dx, None, None, None, dlnw, dlnb, dproj, None


def embed_tokens(tokens: torch.Tensor, table: torch.Tensor, pos: torch.Tensor):
    """GPTPreEncoder.forward (cvap/module/val.py:109-122): returns (x fp32 [b*L, D], eot index i64 [b])."""
    _need(tokens, I64, "embed_tokens.tokens")
    tokens = tokens.contiguous()
    b, L = tokens.shape
    D = table.shape[1]
    assert pos.shape[0] >= L
    x = torch.empty((b * L, D), dtype=F32, device=tokens.device)
    eot = torch.empty((b,), dtype=I64, device=tokens.device)
    call("vipant_embed_tokens", tokens.data_ptr(), table.detach().data_ptr(), pos.detach().contiguous().data_ptr(),
         x.data_ptr(), eot.data_ptr(), b, L, D, _stream())
    return x, eot


def l2_normalize(x: torch.Tensor) -> torch.Tensor:
    """x / ||x|| for pre-computed features (cvap/model/cvalp.py:45-46); no gradient path (inputs are data)."""
    _need(x, F32, "l2_normalize.x")
    x = x.contiguous()
    out = torch.empty_like(x)
    norm = torch.empty((x.shape[0],), dtype=F32, device=x.device)
    call("vipant_l2norm_fwd", x.data_ptr(), out.data_ptr(), norm.data_ptr(), x.shape[0], x.shape[1], _stream())
    return out


def retrieval_ranks(x1: torch.Tensor, x2: torch.Tensor, gold: torch.Tensor, want_top1: bool = False):
    """Rank of the gold candidates of every query without sorting (cvap/module/decoder/loss_head.py:113-118, 141-160):
    x1 [N1, E], x2 [N2, E] fp32 L2-normalised, gold int [N1] or [N1, G] -> ranks int32 of gold's shape
    (= torch.where((x1 @ x2.t()).argsort(descending=True) == gold)[1]) and, optionally, top1 int32 [N1]."""
    _need(x1, F32, "retrieval.x1"); _need(x2, F32, "retrieval.x2")
    x1, x2 = x1.contiguous(), x2.contiguous()
    if gold.device != x1.device or gold.dtype != torch.int32:
        gold = gold.to(device=x1.device, dtype=torch.int32)
    shape = tuple(gold.shape)
    gold2 = gold.reshape(x1.shape[0], -1).contiguous()
    N1, E = x1.shape
    N2, G = x2.shape[0], gold2.shape[1]
    ranks = torch.empty((N1, G), dtype=torch.int32, device=x1.device)
    top1 = torch.empty((N1,), dtype=torch.int32, device=x1.device) if want_top1 else None
    ws = scratch("retrieval", query("vipant_retrieval_workspace_bytes", N1, N2, E, G), x1.device)
    call("vipant_retrieval_ranks", x1.data_ptr(), x2.data_ptr(), gold2.data_ptr(), ranks.data_ptr(), _ptr(top1), N1, N2, E, G,
         ws.data_ptr(), ws.numel(), _stream())
    ranks = ranks.reshape(shape)
    return (ranks, top1) if want_top1 else ranks


class L2NormFn(torch.autograd.Function):
    """x / ||x|| (cvap/module/decoder/loss_head.py:272-273) with its backward, for un-normalised head outputs."""

    @staticmethod
    def forward(ctx, x):
        _need(x, F32, "l2norm.x")
        x = x.contiguous()
        out = torch.empty_like(x)
        norm = torch.empty((x.shape[0],), dtype=F32, device=x.device)
        call("vipant_l2norm_fwd", x.data_ptr(), out.data_ptr(), norm.data_ptr(), x.shape[0], x.shape[1], _stream())
        ctx.save_for_backward(out, norm)
        return out

    @staticmethod
    def backward(ctx, dout):
        out, norm = ctx.saved_tensors
        dout = dout.contiguous()
        dx = torch.empty_like(out)
        call("vipant_l2norm_bwd", dout.data_ptr(), out.data_ptr(), norm.data_ptr(), dx.data_ptr(), None, out.shape[0],
             out.shape[1], _stream())
        return dx


# ---------------------------------------------------------------------------------- InfoNCE
class InfoNCEFn(torch.autograd.Function):
    """CELossHead.forward (cvap/module/decoder/loss_head.py:265-284) on L2-normalised fp32 features.

    x1, x2: [B, E] -- the (all-gathered) global batch.  Gradients are produced only for rows
    [row0, row0 + nrows): the slice this replica owns; other rows get zero (their owners compute them).
    `grad_scale` pre-multiplies the slice gradients (replicas whose parameter gradients are averaged set it
    to the world size so that the mean over ranks equals the full-batch gradient)."""

    @staticmethod
    def forward(ctx, x1, x2, logit_scale, scale_max, row0, nrows, grad_scale):
        _need(x1, F32, "infonce.x1"); _need(x2, F32, "infonce.x2")
        x1, x2 = x1.contiguous(), x2.contiguous()
        B, E = x1.shape
        dev = x1.device
        need = ctx.needs_input_grad
        want = need[0] or need[1] or need[2]
        # (gradients for a strip of a large batch -- one rank of an N-GPU step -- need a third of the workspace: no B x B matrices)
        ws = scratch("infonce", query("vipant_infonce_strip_workspace_bytes", B, E, int(nrows)) if want
                     else query("vipant_infonce_workspace_bytes", B, E), dev)
        loss = torch.empty((1,), dtype=F32, device=dev)
        d1 = torch.empty((nrows, E), dtype=F32, device=dev) if want else None
        d2 = torch.empty((nrows, E), dtype=F32, device=dev) if want else None
        dls = torch.empty((1,), dtype=F32, device=dev) if want else None
        ls = logit_scale.detach().reshape(1).to(F32)
        call("vipant_infonce_fwd_bwd", x1.data_ptr(), x2.data_ptr(), ls.data_ptr(), float(scale_max or 0.0),
             loss.data_ptr(), _ptr(d1), _ptr(d2), _ptr(dls), float(grad_scale), B, E, int(row0), int(nrows),
             ws.data_ptr(), ws.numel(), _stream())
        if want:
            ctx.save_for_backward(d1, d2, dls)
            ctx.meta = (B, E, int(row0), int(nrows), tuple(logit_scale.shape))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        d1, d2, dls = ctx.saved_tensors
        B, E, row0, nrows, ls_shape = ctx.meta
        need = ctx.needs_input_grad

        unit = dloss.dim() == 0 and dloss.data_ptr() == unit_grad(dloss.device).data_ptr()      # the trainer's cached 1.0

        def expand(d):
            if row0 == 0 and nrows == B:         # one replica: the slice is the batch (one launch instead of fill + mul + copy)
                return d if unit else d * dloss
            full = torch.zeros((B, E), dtype=F32, device=d.device)
            full[row0:row0 + nrows] = d * dloss
            return full
        return (expand(d1) if need[0] else None, expand(d2) if need[1] else None,
                (dls if unit else dls * dloss).reshape(ls_shape) if need[2] else None, None, None, None, None)


class InfoNCEMultiMeta:
    """The non-tensor arguments of InfoNCEMultiFn: `pairs` [(a, b)] indexes the operand list, `scale_max` / `weights` are per pair;
    rows [row0, row0 + nrows) get gradients, pre-multiplied by `grad_scale` (InfoNCEFn's conventions).  After the forward
    `losses` is the fp32 device vector [npair + 1]: the unweighted loss of each pair, then the weighted total."""

    def __init__(self, pairs, scale_max, weights, row0, nrows, grad_scale=1.0):
        self.pairs = [(int(a), int(b)) for a, b in pairs]
        self.scale_max = [float(s or 0.0) for s in scale_max]
        self.weights = [float(w) for w in weights]
        if not (len(self.pairs) == len(self.scale_max) == len(self.weights)):
            raise _ffi.VipantError("infonce_multi: pairs, scale_max and weights differ in length")
        self.row0, self.nrows, self.grad_scale = int(row0), int(nrows), float(grad_scale)
        self.losses = None


class InfoNCEMultiFn(torch.autograd.Function):
    """VACELossHead.forward (cvap/module/decoder/loss_head.py:572-598) as ONE node: sum_k w_k InfoNCE(x[a_k], x[b_k]) over L2-normalised
    fp32 operands [B, E] that the pairs share.  `apply(meta, *operands, *logit_scales)`: len(meta.pairs) raw logit scales follow the
    operands.  An operand that needs no gradient (precomputed features) gets none computed."""

    @staticmethod
    def forward(ctx, meta, *tensors):
        npair = len(meta.pairs)
        nop = len(tensors) - npair
        xs = [t.contiguous() for t in tensors[:nop]]
        for i, x in enumerate(xs):
            _need(x, F32, f"infonce_multi.x[{i}]")
            if x.shape != xs[0].shape or x.dim() != 2:
                raise _ffi.VipantError(f"infonce_multi: operand {i} is {tuple(x.shape)}, operand 0 {tuple(xs[0].shape)}")
        B, E = xs[0].shape
        dev = xs[0].device
        need = ctx.needs_input_grad[1:]
        nrows = meta.nrows
        want = any(need) and nrows > 0
        wants = [want and need[i] and any(i in p for p in meta.pairs) for i in range(nop)]
        nbytes = query("vipant_infonce_multi_workspace_bytes", B, E, nop, npair, nrows if want else 0)
        if nbytes == 0:
            raise _ffi.VipantError(f"infonce_multi: {nop} operands / {npair} pairs (1 to 5 each)")
        ws = scratch("infonce_multi", nbytes, dev)
        losses = torch.empty((npair + 1,), dtype=F32, device=dev)
        dxs = [torch.empty((nrows, E), dtype=F32, device=dev) if w else None for w in wants]
        dls = torch.empty((npair,), dtype=F32, device=dev) if want else None
        ls = torch.stack([t.detach().reshape(()).to(F32) for t in tensors[nop:]])
        ptrs = lambda ts: (C.c_void_p * len(ts))(*[_ptr(t) for t in ts])
        i32s = lambda v: (C.c_int32 * len(v))(*v)
        f32s = lambda v: (C.c_float * len(v))(*v)
        call("vipant_infonce_multi_fwd_bwd", ptrs(xs), nop, i32s([a for a, _ in meta.pairs]), i32s([b for _, b in meta.pairs]), npair,
             ls.data_ptr(), f32s(meta.scale_max), f32s(meta.weights), losses.data_ptr(), ptrs(dxs), _ptr(dls), meta.grad_scale,
             B, E, meta.row0, nrows, ws.data_ptr(), ws.numel(), _stream())
        meta.losses = losses
        if want:
            ctx.save_for_backward(dls, *[d for d in dxs if d is not None])
            ctx.meta = (B, E, meta.row0, nrows, nop, [d is not None for d in dxs], [tuple(t.shape) for t in tensors[nop:]])
        return losses[npair].reshape(())

    @staticmethod
    def backward(ctx, dloss):
        dls, *have = ctx.saved_tensors
        B, E, row0, nrows, nop, present, ls_shapes = ctx.meta
        need = ctx.needs_input_grad[1:]
        unit = dloss.dim() == 0 and dloss.data_ptr() == unit_grad(dloss.device).data_ptr()      # the trainer's cached 1.0
        have = iter(have)
        dxs = [next(have) if p else None for p in present]

        def expand(d):
            if row0 == 0 and nrows == B:         # one replica: the slice is the batch
                return d if unit else d * dloss
            full = torch.zeros((B, E), dtype=F32, device=d.device)
            full[row0:row0 + nrows] = d * dloss
            return full
        dl = dls if unit else dls * dloss
        return (None, *[expand(dxs[i]) if need[i] and dxs[i] is not None else None for i in range(nop)],
                *[dl[k].reshape(s) if need[nop + k] else None for k, s in enumerate(ls_shapes)])


# ---------------------------------------------------------------------------------- LARS
class LarsState:
    """Device-side pointer tables for vipant_lars_step (cvap/module/lars.py:43-72); built once per optimizer.

    The per-step inputs -- gradient pointers and learning rates -- reach the device through two alternating PINNED host
    buffers and stream-ordered copies: the host never waits for the stream here (a `torch.tensor(list, device=...)` per step
    is a pageable copy, i.e. a stream synchronisation in the middle of the training loop)."""

    def __init__(self, params: Sequence[torch.Tensor], adapt: Sequence[bool]):
        self.params = list(params)
        dev = self.params[0].device
        n = len(self.params)
        self.mu = [torch.zeros_like(p) for p in self.params]
        self.n = torch.tensor([p.numel() for p in self.params], dtype=I64, device=dev)
        self.adapt = torch.tensor([int(a) for a in adapt], dtype=torch.int32, device=dev)
        self.p_ptrs = torch.tensor([p.data_ptr() for p in self.params], dtype=I64, device=dev)
        self.mu_ptrs = torch.tensor([m.data_ptr() for m in self.mu], dtype=I64, device=dev)
        self.ws = torch.empty((query("vipant_lars_workspace_bytes", n),), dtype=torch.uint8, device=dev)
        # gradient pointers (n x int64) and learning rates (n x fp32) in ONE staging buffer: one host-to-device copy per step
        self.stage = torch.empty((12 * n,), dtype=torch.uint8, device=dev)
        self.g_ptrs = self.stage[:8 * n].view(I64)
        self.lr = self.stage[8 * n:].view(F32)
        self._host = [(torch.empty((12 * n,), dtype=torch.uint8).pin_memory(), None) for _ in range(2)] if dev.type == "cuda" else None
        self._turn = 0

    def step(self, grads: Sequence[torch.Tensor], lrs: Sequence[float], weight_decay: float, momentum: float, eta: float):
        for p, g in zip(self.params, grads):
            assert g.is_contiguous() and g.dtype == F32 and g.shape == p.shape
        hb, ev = self._host[self._turn]
        if ev is not None:
            ev.synchronize()             # the copy issued from this buffer two steps ago (long done)
        n = len(self.params)
        hb[:8 * n].view(I64).copy_(torch.tensor([g.data_ptr() for g in grads], dtype=I64))
        hb[8 * n:].view(F32).copy_(torch.tensor(list(lrs), dtype=F32))
        self.stage.copy_(hb, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._host[self._turn] = (hb, ev)
        self._turn ^= 1
        call("vipant_lars_step", self.p_ptrs.data_ptr(), self.g_ptrs.data_ptr(), self.mu_ptrs.data_ptr(), self.n.data_ptr(),
             self.adapt.data_ptr(), self.lr.data_ptr(), len(self.params), float(weight_decay), float(momentum), float(eta),
             self.ws.data_ptr(), self.ws.numel(), _stream())


# ---------------------------------------------------------------------------------- Barlow Twins head
def batchnorm_fwd(x: torch.Tensor, gamma=None, beta=None, *, relu: bool = False, running_mean=None, running_var=None,
                  num_batches_tracked=None, momentum: float = 0.1, eps: float = 1e-5):
    """nn.BatchNorm1d in training mode over the rows of x (fp32 [M, N]) [+ ReLU] -> (y bf16 [M, N], mean, rstd fp32 [N]).
    The running statistics (optional buffers) are updated in the same launches."""
    _need(x, F32, "batchnorm_fwd.x")
    M, N = x.shape
    y = torch.empty((M, N), dtype=BF16, device=x.device)
    mean, rstd = _stats(N, x.device)
    ws = scratch("batchnorm", query("vipant_batchnorm_workspace_bytes", M, N), x.device)
    call("vipant_batchnorm_fwd", x.data_ptr(), x.stride(0), _ptr(gamma), _ptr(beta), int(relu), y.data_ptr(), mean.data_ptr(),
         rstd.data_ptr(), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), float(momentum), float(eps), M, N,
         ws.data_ptr(), ws.numel(), _stream())
    return y, mean, rstd


def batchnorm_bwd(dy: torch.Tensor, x: torch.Tensor, mean, rstd, gamma=None, beta=None, *, relu: bool = False, dgamma=None,
                  dbeta=None, row0: int = 0, nrows: Optional[int] = None, accumulate: bool = False) -> torch.Tensor:
    """dx bf16 [M, N] of batchnorm_fwd from dy fp32 [M, N]; dgamma / dbeta (+)= their sums over rows [row0, row0 + nrows)."""
    _need(dy, F32, "batchnorm_bwd.dy"); _need(x, F32, "batchnorm_bwd.x")
    M, N = x.shape
    nrows = M - row0 if nrows is None else nrows
    dx = torch.empty((M, N), dtype=BF16, device=x.device)
    ws = scratch("batchnorm", query("vipant_batchnorm_workspace_bytes", M, N), x.device)
    call("vipant_batchnorm_bwd", dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), mean.data_ptr(), rstd.data_ptr(),
         _ptr(gamma), _ptr(beta), int(relu), dx.data_ptr(), _ptr(dgamma), _ptr(dbeta), int(row0), int(nrows), int(accumulate),
         M, N, ws.data_ptr(), ws.numel(), _stream())
    return dx


def barlow_loss(c: torch.Tensor, M: int, lambd: float, *, grad_scale: Optional[torch.Tensor] = None, want_grad: bool = False):
    """Cross-correlation loss of c fp32 [N, N] = zn1^T zn2 (un-scaled, M rows) -> (fp32 [3] = loss, on, off; G; G^T).
    G = d loss / d c * grad_scale / M in bf16 (None unless want_grad); grad_scale: device fp32 scalar (the upstream gradient)."""
    _need(c, F32, "barlow_loss.c")
    N = c.shape[0]
    assert c.shape == (N, N), c.shape
    out = torch.empty((3,), dtype=F32, device=c.device)
    G = torch.empty((N, N), dtype=BF16, device=c.device) if want_grad else None
    Gt = torch.empty((N, N), dtype=BF16, device=c.device) if want_grad else None
    if grad_scale is not None:
        _need(grad_scale, F32, "barlow_loss.grad_scale")
    ws = scratch("barlow_loss", query("vipant_barlow_loss_workspace_bytes", N), c.device)
    call("vipant_barlow_loss", c.data_ptr(), c.stride(0), int(M), float(lambd), out.data_ptr(), _ptr(grad_scale), _ptr(G), _ptr(Gt),
         N, ws.data_ptr(), ws.numel(), _stream())
    return out, G, Gt


def linear_nobias(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """fp32 y [M, out] = x bf16 [M, in] . w^T (nn.Linear(bias=False)), w through cached_bf16."""
    y = torch.empty((x.shape[0], w.shape[0]), dtype=F32, device=x.device)
    return gemm_nt(x, cached_bf16(w), y, epi=EPI_F32)


class BarlowMeta:
    """What BarlowFn needs besides its differentiable inputs: the BN modules (running-statistics buffers, momentum, eps), the
    off-diagonal weight and the rows this replica owns.  `parts` receives the fp32 [3] loss buffer of the last forward."""

    def __init__(self, bns, final_bn, lambd: float, row0: int, nrows: int, want_dx1: bool = True):
        self.bns, self.final_bn, self.lambd, self.row0, self.nrows = list(bns), final_bn, float(lambd), int(row0), int(nrows)
        # whether the caller's view-1 features need a gradient: under replicas x1 reaches BarlowFn through the joint feature
        # all-gather (cat with x2), so `needs_input_grad[0]` is True even for frozen image features
        self.want_dx1 = bool(want_dx1)
        self.parts = None


def _bn_state(bn):
    if bn.momentum is None:
        # torch's cumulative moving average (momentum 1 / num_batches_tracked) is not implemented by the kernel
        raise _ffi.VipantError("BarlowFn: BatchNorm1d(momentum=None) (cumulative moving average) is not supported")
    if not bn.training or not bn.track_running_stats:
        return dict(momentum=bn.momentum, eps=bn.eps)
    return dict(running_mean=bn.running_mean, running_var=bn.running_var, num_batches_tracked=bn.num_batches_tracked,
                momentum=bn.momentum, eps=bn.eps)


class BarlowFn(torch.autograd.Function):
    """BarlowLossHead.forward (cvap/module/decoder/loss_head.py:313-328) in training mode as ONE autograd node.

    x1, x2: fp32 [M, E] un-normalised features (the all-gathered global batch under replicas).  params = (W_0, gamma_0, beta_0,
    ..., W_{L-1}, gamma_{L-1}, beta_{L-1}, W_L): per hidden width a bias-free Linear + BatchNorm1d + ReLU, then the last Linear
    and the affine-free BatchNorm1d.  Both views go through the same weights, view 1 first, so every BN updates its running
    statistics twice.  Feature gradients are produced for rows [row0, row0 + nrows) only (zeros elsewhere; their owners compute
    them), parameter gradients over all M rows -- complete on every replica, like logit_scale's (Barlow head).

    One node rather than one per layer: the tensors between the layers are bf16 forward / fp32 backward (BN output is the next
    contraction's bf16 operand, its gradient the fp32 product of a contraction), and autograd would cast every such gradient
    to the forward dtype through ATen."""

    @staticmethod
    def forward(ctx, x1, x2, meta, *params):
        _need(x1, F32, "barlow.x1"); _need(x2, F32, "barlow.x2")
        L = len(meta.bns)
        Ws, gs, bs = [params[3 * i] for i in range(L)] + [params[3 * L]], [params[3 * i + 1] for i in range(L)], \
            [params[3 * i + 2] for i in range(L)]
        M = x1.shape[0]
        views = []
        for x in (x1, x2):
            h = cast_bf16(x.contiguous())[0]
            hs, ys, st = [h], [], []
            for i in range(L):
                y = linear_nobias(h, Ws[i])
                h, mean, rstd = batchnorm_fwd(y, gs[i], bs[i], relu=True, **_bn_state(meta.bns[i]))
                ys.append(y); st.append((mean, rstd)); hs.append(h)
            z = linear_nobias(h, Ws[L])
            zn, mean, rstd = batchnorm_fwd(z, **_bn_state(meta.final_bn))
            views.append((hs, ys, st, z, zn, (mean, rstd)))
        zn1, zn2 = views[0][4], views[1][4]
        N = zn1.shape[1]
        c = gemm_tn(zn1, zn2, torch.empty((N, N), dtype=F32, device=x1.device))
        loss, _, _ = barlow_loss(c, M, meta.lambd)
        meta.parts = loss
        ctx.meta, ctx.views, ctx.c, ctx.shapes, ctx.weights = meta, views, c, (M, x1.shape[1]), (Ws, gs, bs)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        meta, views, c = ctx.meta, ctx.views, ctx.c
        M, E = ctx.shapes
        L = len(meta.bns)
        need = (ctx.needs_input_grad[0] and meta.want_dx1,) + tuple(ctx.needs_input_grad[1:])
        dev = c.device
        N = c.shape[0]
        _, G, Gt = barlow_loss(c, M, meta.lambd, grad_scale=dloss.detach().reshape(1).to(F32).contiguous(), want_grad=True)
        dzn = [gemm_nt(views[1][4], G, torch.empty((M, N), dtype=F32, device=dev), epi=EPI_F32),     # dzn1 = zn2 . G^T
               gemm_nt(views[0][4], Gt, torch.empty((M, N), dtype=F32, device=dev), epi=EPI_F32)]    # dzn2 = zn1 . G
        del ctx.c
        Ws, gs, bs = ctx.weights
        dW = [torch.empty(w.shape, dtype=F32, device=dev) for w in Ws]
        dg = [torch.empty(g.shape, dtype=F32, device=dev) for g in gs]
        db = [torch.empty(b.shape, dtype=F32, device=dev) for b in bs]
        dxs = [None, None]
        r0, nr = meta.row0, meta.nrows
        for v, (hs, ys, st, z, zn, (zmean, zrstd)) in enumerate(views):
            acc = v > 0
            dy = batchnorm_bwd(dzn[v], z, zmean, zrstd)
            gemm_tn(dy, hs[L], dW[L], accumulate=acc)
            for i in range(L, -1, -1):
                wt = cached_bf16(Ws[i], transpose_only=True)
                if i == 0:
                    if need[v]:
                        dx = (torch.empty((M, E), dtype=F32, device=dev) if (r0 == 0 and nr == M)
                              else torch.zeros((M, E), dtype=F32, device=dev))
                        gemm_nt(dy[r0:r0 + nr], wt, dx[r0:r0 + nr], epi=EPI_F32)
                        dxs[v] = dx
                    break
                dh = gemm_nt(dy, wt, torch.empty((M, Ws[i].shape[1]), dtype=F32, device=dev), epi=EPI_F32)
                mean, rstd = st[i - 1]
                dy = batchnorm_bwd(dh, ys[i - 1], mean, rstd, gs[i - 1], bs[i - 1], relu=True, dgamma=dg[i - 1], dbeta=db[i - 1],
                                   row0=0, nrows=M, accumulate=acc)
                gemm_tn(dy, hs[i - 1], dW[i - 1], accumulate=acc)
        ctx.views = ctx.weights = None
        grads = []
        for i in range(L):
            grads += [dW[i], dg[i], db[i]]
        grads.append(dW[L])
        grads = [g if need[3 + k] else None for k, g in enumerate(grads)]
        return (dxs[0], dxs[1], None, *grads)


# ---------------------------------------------------------------------------------- classification heads
def _ls_scalar(logit_scale: Optional[torch.Tensor], device):
    return None if logit_scale is None else logit_scale.detach().reshape(1).to(device=device, dtype=F32)


def softmax_ce(z: torch.Tensor, labels: torch.Tensor, logit_scale: torch.Tensor, *, C: Optional[int] = None, row0: int = 0,
               nrows: Optional[int] = None, grad_scale: float = 1.0, want_grad: bool = True, ldd: Optional[int] = None,
               want_pred: bool = True):
    """nn.CrossEntropyLoss()(exp(logit_scale) * z[:, :C], labels) over rows [row0, row0 + nrows) of the un-scaled fp32 logits
    z [B, ldz] -> (loss fp32 [1], dz bf16 [B, ldd] | None, dscale fp32 [1] | None, pred int32 [B] | None).  The loss is the
    scored rows' share of the batch mean (denominator B); rows outside the range are not written in dz / pred."""
    _need(z, F32, "softmax_ce.z"); _need(labels, I64, "softmax_ce.labels")
    B = z.shape[0]
    C = z.shape[1] if C is None else int(C)
    nrows = B - row0 if nrows is None else int(nrows)
    ldd = (z.shape[1] if ldd is None else int(ldd))
    dev = z.device
    loss = torch.empty((1,), dtype=F32, device=dev)
    dz = torch.empty((B, ldd), dtype=BF16, device=dev) if want_grad else None
    dscale = torch.empty((1,), dtype=F32, device=dev) if want_grad else None
    pred = torch.empty((B,), dtype=torch.int32, device=dev) if want_pred else None
    ws = scratch("classify", query("vipant_softmax_ce_workspace_bytes", nrows), dev)
    call("vipant_softmax_ce", z.data_ptr(), z.stride(0), labels.data_ptr(), _ls_scalar(logit_scale, dev).data_ptr(), loss.data_ptr(),
         _ptr(dz), ldd, _ptr(dscale), _ptr(pred), int(row0), nrows, float(grad_scale), B, C, ws.data_ptr(), ws.numel(), _stream())
    return loss, dz, dscale, pred


def bce_logits(z: torch.Tensor, targets: torch.Tensor, logit_scale: Optional[torch.Tensor], *, C: Optional[int] = None,
               row0: int = 0, nrows: Optional[int] = None, grad_scale: float = 1.0, want_grad: bool = True,
               ldd: Optional[int] = None, want_prob: bool = False):
    """nn.BCEWithLogitsLoss()(exp(logit_scale) * z[:, :C], targets) (logit_scale None: scale 1) -> (loss fp32 [1], dz bf16
    [B, ldd] | None, dscale fp32 [1] | None, prob fp32 [B, C] | None = sigmoid of the scaled logits).  targets uint8 [B, C]."""
    _need(z, F32, "bce_logits.z"); _need(targets, torch.uint8, "bce_logits.targets")
    return _bce("vipant_bce_logits", z, targets, logit_scale, C, row0, nrows, grad_scale, want_grad, ldd, want_prob)


def bce_logits_soft(z: torch.Tensor, targets: torch.Tensor, logit_scale: Optional[torch.Tensor], *, C: Optional[int] = None,
                    row0: int = 0, nrows: Optional[int] = None, grad_scale: float = 1.0, want_grad: bool = True,
                    ldd: Optional[int] = None, want_prob: bool = False):
    """bce_logits against soft targets fp32 [B, C] (mixup's lam y + (1 - lam) y'; not clamped to [0, 1]).  Targets that are
    exactly 0 or 1 give bce_logits' bits."""
    _need(z, F32, "bce_logits_soft.z"); _need(targets, F32, "bce_logits_soft.targets")
    return _bce("vipant_bce_logits_soft", z, targets, logit_scale, C, row0, nrows, grad_scale, want_grad, ldd, want_prob)


def _bce(entry, z, targets, logit_scale, C, row0, nrows, grad_scale, want_grad, ldd, want_prob):
    B = z.shape[0]
    C = z.shape[1] if C is None else int(C)
    assert targets.shape[0] == B and targets.shape[1] >= C, (z.shape, targets.shape)
    nrows = B - row0 if nrows is None else int(nrows)
    ldd = (z.shape[1] if ldd is None else int(ldd))
    dev = z.device
    ls = _ls_scalar(logit_scale, dev)
    loss = torch.empty((1,), dtype=F32, device=dev)
    dz = torch.empty((B, ldd), dtype=BF16, device=dev) if want_grad else None
    dscale = torch.empty((1,), dtype=F32, device=dev) if (want_grad and ls is not None) else None
    prob = torch.empty((B, C), dtype=F32, device=dev) if want_prob else None
    ws = scratch("classify", query("vipant_bce_logits_workspace_bytes", nrows), dev)
    call(entry, z.data_ptr(), z.stride(0), targets.data_ptr(), targets.stride(0), _ptr(ls), loss.data_ptr(), _ptr(dz),
         ldd, _ptr(dscale), _ptr(prob), C, int(row0), nrows, float(grad_scale), B, C, ws.data_ptr(), ws.numel(), _stream())
    return loss, dz, dscale, prob


def multihot_mix(ids: torch.Tensor, offsets: torch.Tensor, C: int, *, outputs: Optional[int] = None, mix=None) -> torch.Tensor:
    """Ragged class-id lists -> (soft) multi-hot targets fp32 [b, C] (vipant_multihot_mix).  ids int32 [total], offsets int32
    [nsrc + 1] (row r's classes are ids[offsets[r] : offsets[r + 1]]), b = outputs (default nsrc); mix = (index int32 [b] with values
    in [-1, nsrc), lambda fp32 [b]) or None: y[i] = lam_i [L_i] + (1 - lam_i) [L_index[i]], the bits of ASMonitor.soft_labels on the
    dense rows; without mix, or where index is -1, exactly the {0, 1} row."""
    _need(ids, torch.int32, "multihot_mix.ids"); _need(offsets, torch.int32, "multihot_mix.offsets")
    if ids.dim() != 1 or offsets.dim() != 1 or offsets.numel() < 2:
        raise _ffi.VipantError(f"multihot_mix: ids [total] and offsets [nsrc + 1] expected, got {tuple(ids.shape)} / {tuple(offsets.shape)}")
    nsrc = offsets.numel() - 1
    b = nsrc if outputs is None else int(outputs)
    dev = ids.device
    total = ids.numel()
    if total == 0:                                                  # every list empty: the entry point still wants a pointer
        ids = torch.zeros((1,), dtype=torch.int32, device=dev)
    index = lam = None
    if mix is not None:
        index = mix[0].to(device=dev, dtype=torch.int32).contiguous()
        lam = mix[1].to(device=dev, dtype=F32).contiguous()
        if index.shape != (b,) or lam.shape != (b,):
            raise _ffi.VipantError(f"multihot_mix: mix index / lambda must have shape [{b}], got {tuple(index.shape)} / {tuple(lam.shape)}")
    y = torch.empty((max(b, 0), int(C)), dtype=F32, device=dev)
    call("vipant_multihot_mix", ids.data_ptr(), total, offsets.data_ptr(), _ptr(index), _ptr(lam), y.data_ptr(), nsrc, b, int(C),
         _stream())
    return y


_padded: Dict[tuple, tuple] = {}


def padded_classifier(w: torch.Tensor, bias: Optional[torch.Tensor], Cp: int):
    """The last Linear of a classification head with its class dimension padded to Cp rows: (bf16 [Cp, K], its transpose bf16
    [K, Cp], fp32 bias [Cp] | None), rows / entries C .. Cp-1 zero.  vipant_gemm_nt needs N % 4 == 0 and K % 64 == 0 and the
    input-gradient contraction has the classes as K.  The fp32 staging copies persist per weight (their pad stays zero) and are
    refreshed, with one cast launch, when the parameter's version changes."""
    key = (w.data_ptr(), tuple(w.shape), Cp, None if bias is None else bias.data_ptr())
    ver = (w._version, None if bias is None else bias._version)
    hit = _padded.get(key)
    if hit is None:
        while len(_padded) >= 64:
            _padded.pop(next(iter(_padded)))
        hit = _padded[key] = dict(w32=torch.zeros((Cp, w.shape[1]), dtype=F32, device=w.device),
                                  b32=None if bias is None else torch.zeros((Cp,), dtype=F32, device=w.device),
                                  ver=None, keep=(w.untyped_storage(), None if bias is None else bias.untyped_storage()))
    if hit["ver"] != ver:
        C = w.shape[0]
        hit["w32"][:C].copy_(w.detach())
        if bias is not None:
            hit["b32"][:C].copy_(bias.detach())
        hit["wb"], hit["wt"] = cast_bf16(hit["w32"], transpose=True)
        hit["ver"] = ver
    return hit["wb"], hit["wt"], hit["b32"]


class ClassifierMeta:
    """What ClassifierFn needs besides its differentiable inputs: the loss ("ce": int64 labels [B]; "bce": uint8 multi-hot
    targets [B, C]; "bce_soft": fp32 soft targets [B, C]), the class count, 1 / world for a replica's share of the gradient, and what the eval path wants back.
    `pred` / `prob` receive the arg-max columns / sigmoid scores of the last forward."""

    def __init__(self, kind: str, nclass: int, grad_scale: float = 1.0, want_pred: bool = False, want_prob: bool = False):
        assert kind in ("ce", "bce", "bce_soft"), kind
        self.kind, self.nclass, self.grad_scale = kind, int(nclass), float(grad_scale)
        self.want_pred, self.want_prob = bool(want_pred), bool(want_prob)
        self.pred = self.prob = None


class ClassifierFn(torch.autograd.Function):
    """ClassificationHead.forward / BCELossHead.forward (cvap/module/decoder/loss_head.py:409-419, loss_more.py:133-143) as ONE
    autograd node: [LayerNorm -> Linear] x (L + 1), the temperature and the loss.

    x fp32 [B, E]; target: labels or multi-hot targets (see ClassifierMeta); logit_scale: the log temperature (a parameter, a
    plain tensor, or None for scale 1); params = (ln_w_0, ln_b_0, W_0, b_0, ..., ln_w_L, ln_b_L, W_L, b_L | None).  The last
    Linear runs with its class dimension padded to a multiple of 64 (padded_classifier); the loss kernel reads the C valid
    columns and writes dz with zero pad columns, so the pad never enters the loss or a gradient.  LayerNorm, the contractions,
    the bias sums (from the weight-gradient contraction's operand tiles and the LayerNorm backward's `dx_colsum`) are the
    library's; forward and loss gradient are one pass (vipant_softmax_ce / vipant_bce_logits), the backward is contractions."""

    @staticmethod
    def forward(ctx, x, target, logit_scale, meta, *params):
        _need(x, F32, "classifier.x")
        x = x.contiguous()
        L = len(params) // 4 - 1
        dev, B, C = x.device, x.shape[0], meta.nclass
        Cp = (C + 63) // 64 * 64
        need = ctx.needs_input_grad
        want = any(need)
        h, saved = x, []
        for i in range(L + 1):
            g, b, W, bias = params[4 * i:4 * i + 4]
            y, _, mean, rstd = layernorm_fwd(h, g, b)
            saved.append((h, y, mean, rstd))
            if i < L:
                h = gemm_nt(y, cached_bf16(W), torch.empty((B, W.shape[0]), dtype=F32, device=dev), bias=bias, epi=EPI_F32)
            else:
                wb, wt, b32 = padded_classifier(W, bias, Cp)
                z = gemm_nt(y, wb, torch.empty((B, Cp), dtype=F32, device=dev), bias=b32, epi=EPI_F32)
        if meta.kind == "ce":
            loss, dz, dls, pred = softmax_ce(z, target, logit_scale, C=C, grad_scale=meta.grad_scale, want_grad=want,
                                             want_pred=meta.want_pred)
            meta.pred = pred
        else:
            bce = bce_logits_soft if meta.kind == "bce_soft" else bce_logits
            loss, dz, dls, prob = bce(z, target, logit_scale, C=C, grad_scale=meta.grad_scale, want_grad=want, want_prob=meta.want_prob)
            meta.prob = prob
        if want:
            ctx.saved, ctx.dz, ctx.dls, ctx.wt, ctx.params = saved, dz, dls, wt, params
            ctx.shapes = (L, C, Cp, None if logit_scale is None else tuple(logit_scale.shape))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, dloss):
        L, C, Cp, ls_shape = ctx.shapes
        saved, params, need = ctx.saved, ctx.params, ctx.needs_input_grad
        dev = ctx.dz.device
        B = ctx.dz.shape[0]
        grads = [None] * len(params)
        dy_b, dx = ctx.dz, None                       # bf16 gradient of layer i's Linear output
        for i in range(L, -1, -1):
            g, b, W, bias = params[4 * i:4 * i + 4]
            h, y, mean, rstd = saved[i]
            K = W.shape[1]
            rows = Cp if i == L else W.shape[0]
            dW = torch.empty((rows, K), dtype=F32, device=dev)
            db = torch.empty((rows,), dtype=F32, device=dev) if (i == L and bias is not None) else None
            gemm_tn(dy_b, y, dW, a_colsum=db)                         # hidden layers' bias sums came from the LayerNorm backward
            grads[4 * i + 2] = dW[:W.shape[0]]
            if db is not None:
                grads[4 * i + 3] = db[:W.shape[0]]
            wt = ctx.wt if i == L else cached_bf16(W, transpose_only=True)
            dyl = gemm_nt(dy_b, wt, torch.empty((B, K), dtype=F32, device=dev), epi=EPI_F32)
            dg, dbeta = torch.empty_like(g), torch.empty_like(b)
            if i > 0:
                dy_b = torch.empty((B, K), dtype=BF16, device=dev)
                dbias = torch.empty((K,), dtype=F32, device=dev)      # = d bias of Linear i - 1 (column sums of its output gradient)
                layernorm_bwd(dyl, h, mean, rstd, g, dx_bf16=dy_b, dgamma=dg, dbeta=dbeta, dx_colsum=dbias)
                grads[4 * (i - 1) + 3] = dbias
            elif need[0]:
                dx = torch.empty((B, K), dtype=F32, device=dev)
                layernorm_bwd(dyl, h, mean, rstd, g, dx=dx, dgamma=dg, dbeta=dbeta)
            else:
                layernorm_bwd(dyl, h, mean, rstd, g, dx_bf16=torch.empty((B, K), dtype=BF16, device=dev), dgamma=dg, dbeta=dbeta)
            grads[4 * i], grads[4 * i + 1] = dg, dbeta
        dls = ctx.dls
        ctx.saved = ctx.dz = ctx.params = ctx.wt = None
        unit = dloss.dim() == 0 and dloss.data_ptr() == unit_grad(dloss.device).data_ptr()
        if not unit:                                   # an upstream factor other than the trainer's cached 1.0
            dx = None if dx is None else dx * dloss
            grads = [None if t is None else t * dloss for t in grads]
            dls = None if dls is None else dls * dloss
        grads = [t if (t is not None and need[4 + k]) else None for k, t in enumerate(grads)]
        dls = dls.reshape(ls_shape) if (dls is not None and need[2] and ls_shape is not None) else None
        return (dx, None, dls, None, *grads)
