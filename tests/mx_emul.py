"""Emulations of the e4m3 operand formats that more than one test file needs (tests/test_fp8_gpu.py, tests/test_gemm_nt_gpu.py): the
dequantisers, the block-uniform quantiser (one exponent per aligned block of 32 rows x 32 columns) and the check of a block-uniform
form left by a producer.  `ops` is vipant_amd.ops (the MX scale layout comes from there)."""
import torch


def dequant(q_u8, s_u8):
    return q_u8.view(torch.float8_e4m3fn).float() * torch.exp2(s_u8.float() - 127)[:, None]


def mx_scales(ops, s_tiled, M, K):
    """the library's scale array (MX layout) -> scale bytes [M, K / 32]"""
    return s_tiled[ops.mx_scale_index(M, K, s_tiled.device)]


def dequant_mx(ops, q_u8, s_tiled):
    M, K = q_u8.shape
    sc = torch.exp2(mx_scales(ops, s_tiled, M, K).float() - 127)
    return (q_u8.view(torch.float8_e4m3fn).float().view(M, K // 32, 32) * sc[:, :, None]).view(M, K)


def emulate_quant_mx32(x_bf16):
    """block-uniform format (round 6): one exponent per aligned block of 32 rows x 32 columns; (q float8 [M, K], scale bytes [M, K / 32])."""
    M, K = x_bf16.shape
    Mp = (M + 31) // 32 * 32
    x = torch.zeros(Mp, K, dtype=torch.float32, device=x_bf16.device)
    x[:M] = x_bf16.float()
    blk = x.view(Mp // 32, 32, K // 32, 32)
    amax = blk.abs().amax(dim=(1, 3))
    e = torch.floor(torch.log2(amax.clamp_min(1e-38))) - 8
    e = torch.where(amax * torch.exp2(-e) > 448, e + 1, e)
    e = torch.where(amax > 0, e, torch.full_like(e, -127)).clamp(-127, 127)
    q = (blk * torch.exp2(-e)[:, None, :, None]).to(torch.float8_e4m3fn).view(Mp, K)[:M]
    s = (e + 127).to(torch.uint8)[:, None, :].expand(Mp // 32, 32, K // 32).reshape(Mp, K // 32)[:M]
    return q, s


def check_block_uniform_form(ops, em, ref_bf16, slack):
    """(bytes, scales) left by a producer for the bf16 matrix `ref_bf16`: scales uniform over aligned 32 x 32 blocks, never below
    what the block's largest element needs (nothing saturates) and at most `slack` binades above it (the producers take the scale
    from a bound they have in registers, not from the exact maximum), and the bytes exactly ref / 2^e rounded to e4m3."""
    M, N = ref_bf16.shape
    s = mx_scales(ops, em[1], M, N).int()
    _, s_min = emulate_quant_mx32(ref_bf16)
    Mp = (M + 31) // 32 * 32
    pad = torch.zeros(Mp, N // 32, dtype=torch.int32, device=s.device); pad[:M] = s
    pad[M:] = pad[(M - 1) // 32 * 32]                                  # rows beyond M: whatever the block has
    blk = pad.view(Mp // 32, 32, N // 32)
    assert torch.equal(blk.amax(dim=1), blk.amin(dim=1))                # one scale per block
    nz = s_min.int() > 0
    assert bool((s[nz] >= s_min.int()[nz]).all()) and bool((s[nz] <= s_min.int()[nz] + slack).all()), \
        (int((s - s_min.int())[nz].min()), int((s - s_min.int())[nz].max()))
    sc = torch.exp2(s.float() - 127)[:, :, None].expand(M, N // 32, 32).reshape(M, N)
    want = (ref_bf16.float() / sc).to(torch.float8_e4m3fn).view(torch.uint8)
    zero_blk = (~nz)[:, :, None].expand(M, N // 32, 32).reshape(M, N)
    assert torch.equal(em[0][~zero_blk], want[~zero_blk])
    print(f"block-uniform emit: scale - minimal scale: mean {float((s - s_min.int())[nz].float().mean()):.3f} binades")
