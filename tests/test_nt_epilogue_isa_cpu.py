"""The tile epilogue of the ping-pong NT kernels, in the assembly of the shipped build: no full wait (`s_waitcnt vmcnt(0)`) between a
kernel's result stores -- the QuickGELU' epilogues, which load an input per result, request all of them in front of the first store and
await them once (vipant_amd/isa_guard.py: check_gemm_nt_epilogue, run by the build as well).  No GPU needed."""
import re

import pytest

BF16, QUICKGELU_D8, DQUICKGELU, DQUICKGELU_D8 = 0, 6, 4, 7


@pytest.fixture(scope="module")
def isa():
    from vipant_amd import build
    build.build(verbose=False)
    return build.isa_path("gemm_nt.hip")


def test_guard_holds_on_the_shipped_build(isa):
    from vipant_amd import isa_guard
    isa_guard.check_gemm_nt_epilogue(isa)


def test_every_quickgelu_derivative_instance_is_covered(isa):
    """Every gemm_nt_pp_kernel<4 | 7, ...> the library holds is in the guard's table, on both walks, bf16 and e4m3, every emit mode; each
    shows its sixteen 16-byte stores (8-byte ones where only the e4m3 form leaves) with no full wait between them."""
    from vipant_amd import isa_guard
    table = isa_guard.pp_epilogue_waits(isa)
    names = set(re.findall(r"^_ZN\S*gemm_nt_pp_kernelILi([47])ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E\S*:", open(isa).read(), flags=re.M))
    want = {(int(e), int(v), int(s), int(m), int(d)) for e, v, s, m, d in names}
    got = {k for k in table if k[0] in (DQUICKGELU, DQUICKGELU_D8)}
    assert got == want and len(got) >= 14, sorted(want - got)
    # the step's own instantiation (DEEP_GROUPED) and its plain-walk twin, ticket and static; the bf16-input epilogue; the e4m3 towers'
    for key in ((7, 12, 2, 0, 1), (7, 12, 2, 0, 0), (7, 10, 2, 0, 1), (7, 10, 2, 0, 0), (7, 0, 2, 0, 1), (4, 0, 2, 0, 1), (4, 10, 2, 0, 0),
                (7, 0, 1, 0, 0), (7, 0, 1, 1, 0)):
        assert key in got, key
    for key in got:
        before, inside, stores = table[key]
        assert inside == 0, (key, inside)
        assert stores >= 16, (key, stores)


def test_the_other_epilogues_still_show_no_full_wait(isa):
    """The regression in the other direction: the BF16 and QUICKGELU_D8 epilogues only store, and stay free of full waits."""
    from vipant_amd import isa_guard
    table = isa_guard.pp_epilogue_waits(isa)
    for epi in (BF16, QUICKGELU_D8):
        mine = {k: v for k, v in table.items() if k[0] == epi}
        assert len(mine) >= 8, (epi, sorted(mine))
        assert all(v[1] == 0 for v in mine.values()), {k: v for k, v in mine.items() if v[1]}


def test_last_k_tile_of_the_bf16_kernels_has_no_drain(isa):
    """QuickGELU' reads no bias: its bf16 kernels hold exactly as many full waits in front of the first store as their BF16 twins -- the
    twin's bias round trip against the one wait for the inputs, and none inside the K-loop."""
    from vipant_amd import isa_guard
    table = isa_guard.pp_epilogue_waits(isa)
    for key in [k for k in table if k[0] in (DQUICKGELU, DQUICKGELU_D8) and k[2] == 2]:
        twin = (BF16,) + key[1:]
        assert twin in table, key
        assert table[key][0] <= table[twin][0], (key, table[key][0], table[twin][0])


def test_guard_rejects_a_drain_between_the_stores(isa, tmp_path):
    """A guard that cannot fail protects nothing: a full wait put in front of the LAST 16-byte store of the step's QuickGELU' kernel, and
    one put into its K-loop, must each be refused."""
    from vipant_amd import isa_guard
    text = open(isa).read()
    k = re.search(r"^_ZN\S*gemm_nt_pp_kernelILi7ELi12ELi2ELi0ELb1E\S*:", text, flags=re.M)
    end = text.index("s_endpgm", k.start())
    body = text[k.start():end]
    stores = [m.start() for m in re.finditer(r"^\s*global_store_dwordx4\b", body, flags=re.M)]
    assert len(stores) == 16
    bad = tmp_path / "between.s"
    bad.write_text(text[:k.start()] + body[:stores[-1]] + "\n\ts_waitcnt vmcnt(0)\n" + body[stores[-1]:] + text[end:])
    with pytest.raises(AssertionError):
        isa_guard.check_gemm_nt_epilogue(str(bad))
    dma = [m.start() for m in re.finditer(r"^\s*buffer_load_dwordx4\b[^\n]*\blds\b", body, flags=re.M)]
    assert dma and dma[-1] < stores[0]
    bad2 = tmp_path / "kloop.s"
    bad2.write_text(text[:k.start()] + body[:dma[-1]] + "\n\ts_waitcnt vmcnt(0)\n" + body[dma[-1]:] + text[end:])
    with pytest.raises(AssertionError):
        isa_guard.check_gemm_nt_epilogue(str(bad2))
