"""The CPU half of tests/test_attention_gpu.py: the sweep's parameter list reaches every kernel instance, the constructed inputs of
the concentrated-row and masked-key tests have the properties those tests rely on, and the bf16-operand emulation the GPU tests
take their budgets from is the reference function up to bf16 rounding.  No GPU, no kernel: fp64 on the CPU."""
import pytest
import torch

import test_attention_gpu as A


def test_sweep_covers_every_instance():
    A.check_coverage(A.SWEEP)
    assert len(set(A.SWEEP)) == len(A.SWEEP)
    for S in (1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 288, 289, 320, 321, 352, 353, 384, 385, 448, 449):
        assert (S, False) in A.SWEEP and (S, True) in A.SWEEP, S


def test_selection_follows_the_seven_bounds():
    assert A.select(316, False) == (20, 2, False, "bwd1s") and A.select(230, False) == (20, 20, False, "bwd1s")
    assert A.select(316, True) == (20, 2, True, "2pass-8w") and A.select(77, True) == (6, 2, True, "2pass-4w")
    assert A.select(126, False) == (10, 10, False, "2pass-8w") and A.select(200, False) == (14, 2, False, "2pass-8w")
    assert A.select(370, True) == (24, 2, True, "2pass-8w") and A.select(384, False)[0] == 24
    assert A.select(385, False) == (0, 0, False, "stream") and A.select(16, False) == (2, 2, False, "2pass-4w")


@pytest.mark.parametrize("drop", [[176], [97, 112, 128], [385], [448, 512], [225, 256, 288], [384]])
def test_coverage_notices_a_lost_row(drop):
    """Without S = 176 no whole-tile length is left inside NT = 14 / EDGE = 14; the other lists drop a whole row or a streaming property."""
    for causal in (False, True):
        with pytest.raises(AssertionError):
            A.check_coverage([c for c in A.SWEEP if not (c[0] in drop and c[1] == causal)])


@pytest.mark.parametrize("S,causal,gain,i,a,b", A.SPIKY_CASES)
def test_concentrated_rows_premises(S, causal, gain, i, a, b):
    qkv, dout = A.spiky_case(S, gain, i, a, b)
    A.spiky_premises(qkv, dout, S, causal, gain, i, a, b)


@pytest.mark.parametrize("S,i,j", A.MASKED)
def test_masked_key_premises(S, i, j):
    qkv, _ = A.masked_case(S, i, j)
    A.masked_premises(qkv, S, i, j)


@pytest.mark.parametrize("S,causal", [(1, False), (50, True), (97, False), (130, True), (449, False), (449, True)])
def test_emulation_is_the_reference_up_to_bf16(S, causal):
    """Every block of the emulation within 2^-7 of the block's norm of the fp64 reference (bf16 carries 2^-9 per rounding, the
    blocks pass through two or three), lse within fp32 rounding."""
    batch, H = 2, 3
    qkv = A.rnd_cpu(batch * S, 3 * H * 64, seed=1, scale=1.5).to(torch.bfloat16)
    dout = A.rnd_cpu(batch * S, H * 64, seed=2).to(torch.bfloat16)
    qr = qkv.double().requires_grad_()
    ref, rlse = A.ref_attention(qr, batch, S, H, causal)
    ref.backward(dout.double())
    out, lse, dqkv = A.emulate(qkv, dout, batch, S, H, causal)
    A.check_lse("emulation", lse, rlse)
    assert float((out - ref.detach()).norm()) <= 2.0 ** -7 * float(ref.detach().norm())
    for name, blk in A.blocks(dqkv, H).items():
        want = A.blocks(qr.grad, H)[name]
        assert float((blk - want).norm()) <= 2.0 ** -7 * float(want.norm()) + 1e-12, name
