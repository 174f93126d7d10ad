"""Ragged class-id lists -> (soft) multi-hot tagging targets on the device (vipant_multihot_mix, ops.multihot_mix).

The contract is bit-identity, not a tolerance: y equals ASMonitor.soft_labels (torch fp32: lam * y + (1 - lam) * y[partner], each
product and the sum rounded separately) on the dense multi-hot rows built on the host; unmixed rows are exact {0, 1}."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(1, 1, 1), (3, 5, 7), (64, 100, 527)]
SENTINEL = -777.0


def ragged(b, nsrc, C, seed):
    """Lists with duplicates, empty lists, and ids -1 and C that must be ignored -> (ids, offsets, dense [nsrc, C])."""
    g = torch.Generator().manual_seed(seed)
    lists = []
    for r in range(nsrc):
        k = int(torch.randint(0, 5, (1,), generator=g))
        row = torch.randint(0, C, (k,), generator=g).tolist()
        if r % 3 == 0 and row:
            row = row + row[:1]                                         # a duplicate id
        if r % 4 == 1:
            row = [-1] + row + [C]                                      # outside [0, C): ignored
        if r % 5 == 2:
            row = []                                                    # an empty list
        lists.append(row)
    if nsrc > 1:
        lists[-1] = []
    dense = torch.zeros(nsrc, C)
    for r, row in enumerate(lists):
        for c in row:
            if 0 <= c < C:
                dense[r, c] = 1.0
    offsets = [0]
    for row in lists:
        offsets.append(offsets[-1] + len(row))
    ids = torch.tensor([c for row in lists for c in row], dtype=torch.int32)
    return ids, torch.tensor(offsets, dtype=torch.int32), dense, lists


def draws(b, nsrc, seed):
    g = torch.Generator().manual_seed(seed + 1)
    index = torch.randint(0, nsrc, (b,), generator=g).to(torch.int32)
    lam = 0.1 + 0.8 * torch.rand(b, generator=g)
    for i in range(0, b, 3):                                            # every third clip unmixed, as draw_mixup leaves it
        index[i], lam[i] = -1, 1.0
    return index, lam


def want_soft(dense, index, lam, b):
    """ASMonitor.soft_labels over all nsrc dense rows (rows >= b unmixed), on the device like the trainer; the first b rows."""
    from vipant_amd.monitor import ASMonitor
    nsrc = dense.shape[0]
    full_i = torch.full((nsrc,), -1, dtype=torch.int32)
    full_l = torch.ones(nsrc)
    full_i[:b], full_l[:b] = index, lam
    return ASMonitor.soft_labels(dense.to(DEV), full_i, full_l)[:b]


@pytest.mark.parametrize("b,nsrc,C", CASES)
def test_bits_of_soft_labels(b, nsrc, C):
    from vipant_amd import ops
    ids, offsets, dense, lists = ragged(b, nsrc, C, seed=C)
    index, lam = draws(b, nsrc, seed=C)
    if b > 1:
        index[1], lam[1] = nsrc - 1, 1.0                                # lam = 1 with a partner: the clip's own row exactly
    y = ops.multihot_mix(ids.to(DEV), offsets.to(DEV), C, outputs=b, mix=(index, lam))
    assert y.shape == (b, C) and y.dtype == torch.float32
    want = want_soft(dense, index, lam, b)
    assert torch.equal(y, want)
    if b > 1:
        assert torch.equal(y[1], dense[1].to(DEV))
    assert torch.equal(y[0], dense[0].to(DEV))                          # index -1
    assert torch.equal(ops.multihot_mix(ids.to(DEV), offsets.to(DEV), C, outputs=b, mix=(index, lam)), y)
    # without mix arguments: exact {0, 1}, duplicates give 1, empty lists zero rows, -1 and C ignored
    hard = ops.multihot_mix(ids.to(DEV), offsets.to(DEV), C, outputs=b)
    assert torch.equal(hard, dense[:b].to(DEV))
    assert bool(((hard == 0) | (hard == 1)).all())
    every = ops.multihot_mix(ids.to(DEV), offsets.to(DEV), C)
    assert torch.equal(every, dense.to(DEV))
    for r, row in enumerate(lists):
        if not [c for c in row if 0 <= c < C]:
            assert float(every[r].abs().sum()) == 0.0
    if C == 527:                                                        # the trainer's case has what the list is about
        assert any(len(row) != len(set(row)) for row in lists) and any(-1 in row and C in row for row in lists)
        assert bool(((y > 0) & (y < 1)).any())


def test_duplicates_empty_lists_and_ignored_ids_by_hand():
    from vipant_amd import ops
    C = 7
    lists = [[2, 2, 5, 2], [], [-1, 7, 3, 100, -2147483648, 2147483647], [6, 0], [5]]
    ids = torch.tensor([c for row in lists for c in row], dtype=torch.int32, device=DEV)
    offsets = torch.tensor([0, 4, 4, 10, 12, 13], dtype=torch.int32, device=DEV)
    y = ops.multihot_mix(ids, offsets, C).cpu()
    assert y.tolist() == [[0, 0, 1, 0, 0, 1, 0], [0] * 7, [0, 0, 0, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1, 0]]
    index = torch.tensor([4, 3, -1], dtype=torch.int32)
    lam = torch.tensor([0.25, 0.7, 1.0])
    y = ops.multihot_mix(ids, offsets, C, outputs=3, mix=(index, lam)).cpu()
    f = torch.tensor
    assert torch.equal(y[0], f([0, 0, 0.25, 0, 0, 1.0, 0]))             # class 5 in both lists: 0.25 + 0.75
    assert torch.equal(y[1], (f(1.0) - f(0.7)) * f([1.0, 0, 0, 0, 0, 0, 1.0]))
    assert torch.equal(y[2], f([0, 0, 0, 1.0, 0, 0, 0]))
    # mix_index is clamped like the log-mel entry's: nsrc and above -> row nsrc - 1, below -1 -> not mixed
    wild = torch.tensor([5, 1000000, -5], dtype=torch.int32)
    tame = torch.tensor([4, 4, -1], dtype=torch.int32)
    lam = torch.tensor([0.25, 0.7, 0.3])
    got = ops.multihot_mix(ids, offsets, C, outputs=3, mix=(wild, lam))
    assert torch.equal(got, ops.multihot_mix(ids, offsets, C, outputs=3, mix=(tame, lam)))
    assert torch.equal(got[2].cpu(), f([0, 0, 0, 1.0, 0, 0, 0]))        # not mixed: exact whatever lambda says
    with pytest.raises(ops._ffi.VipantError):
        ops.multihot_mix(ids, offsets, C, outputs=3, mix=(tame[:2], lam))
    with pytest.raises(ops._ffi.VipantError, match="no CPU fallback"):
        ops.multihot_mix(ids.cpu(), offsets.cpu(), C)


def _raw(ids_ptr, total, offsets_ptr, index_ptr, lam_ptr, y_ptr, nsrc, b, C):
    from vipant_amd import _ffi, ops
    return _ffi.lib().vipant_multihot_mix(ids_ptr, total, offsets_ptr, index_ptr, lam_ptr, y_ptr, nsrc, b, C, ops._stream())


def test_poisoned_offsets_read_nothing_outside_ids():
    """Decreasing offsets and offsets beyond `total` (or negative): the kernel clamps them into [0, total].  ids sits inside a guard
    of class ids that are valid (NaN-free: int32) but belong to nobody; reading them would switch on classes 0 .. 3."""
    b = nsrc = 4
    C, total, guard = 9, 6, 64
    store = torch.arange(2 * guard + total, dtype=torch.int32, device=DEV) % 4          # guard values: classes 0 .. 3
    store[guard:guard + total] = torch.tensor([5, 6, 7, 8, 5, 6], dtype=torch.int32)
    ids_ptr = store.data_ptr() + 4 * guard
    offsets = torch.tensor([-50, 2, 1, 1000, 6], dtype=torch.int32, device=DEV)        # row 0: [0, 2); 1: decreasing -> empty; 2: [1, 6); 3: [6, 6)
    buf = torch.full((8 + b * C + 8,), SENTINEL, device=DEV)
    assert _raw(ids_ptr, total, offsets.data_ptr(), None, None, buf.data_ptr() + 4 * 8, nsrc, b, C) == 0
    torch.cuda.synchronize()
    y = buf[8:8 + b * C].view(b, C).cpu()
    assert bool(torch.isfinite(y).all())
    assert bool((buf[:8] == SENTINEL).all()) and bool((buf[8 + b * C:] == SENTINEL).all())
    assert float(y[:, :4].abs().sum()) == 0.0                           # nothing from the guard
    assert y[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 0, 0]
    assert y[1].tolist() == [0] * 9
    assert y[2].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    assert y[3].tolist() == [0] * 9
    off2 = torch.tensor([2147483647, -2147483648, 2147483647, 3, -1], dtype=torch.int32, device=DEV)
    assert _raw(ids_ptr, total, off2.data_ptr(), None, None, buf.data_ptr() + 4 * 8, nsrc, b, C) == 0
    torch.cuda.synchronize()
    y = buf[8:8 + b * C].view(b, C).cpu()
    assert float(y[:, :4].abs().sum()) == 0.0
    assert y[0].tolist() == [0] * 9 and y[2].tolist() == [0] * 9 and y[3].tolist() == [0] * 9
    assert y[1].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1]                 # [INT_MIN, INT_MAX) clamps to the whole of ids
    assert bool((buf[:8] == SENTINEL).all()) and bool((buf[8 + b * C:] == SENTINEL).all())


def test_refusals_write_nothing():
    b, nsrc, C = 3, 5, 7
    ids, offsets, _, _ = ragged(b, nsrc, C, seed=5)
    ids, offsets = ids.to(DEV), offsets.to(DEV)
    index = torch.tensor([4, -1, 3], dtype=torch.int32, device=DEV)
    lam = torch.tensor([0.5, 1.0, 0.25], device=DEV)
    buf = torch.full((b * C + 16,), SENTINEL, device=DEV)
    y_ptr = buf.data_ptr() + 4 * 8
    i, o, x, l, n = ids.data_ptr(), offsets.data_ptr(), index.data_ptr(), lam.data_ptr(), ids.numel()
    assert _raw(None, n, o, x, l, y_ptr, nsrc, b, C) != 0               # NULL ids / offsets / y
    assert _raw(i, n, None, x, l, y_ptr, nsrc, b, C) != 0
    assert _raw(i, n, o, x, l, None, nsrc, b, C) != 0
    assert _raw(i, n, o, x, l, y_ptr, nsrc, 0, C) != 0                  # b < 1
    assert _raw(i, n, o, x, l, y_ptr, nsrc, -3, C) != 0
    assert _raw(i, n, o, x, l, y_ptr, 2, b, C) != 0                     # nsrc < b
    assert _raw(i, n, o, x, l, y_ptr, nsrc, b, 0) != 0                  # C < 1
    assert _raw(i, n, o, x, None, y_ptr, nsrc, b, C) != 0               # exactly one of the two mix pointers
    assert _raw(i, n, o, None, l, y_ptr, nsrc, b, C) != 0
    assert _raw(i, -1, o, x, l, y_ptr, nsrc, b, C) != 0                 # total < 0
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert _raw(i, n, o, x, l, y_ptr, nsrc, b, C) == 0
    torch.cuda.synchronize()
    assert bool((buf[:8] == SENTINEL).all()) and bool((buf[8 + b * C:] == SENTINEL).all()) and bool((buf[8:8 + b * C] != SENTINEL).all())
