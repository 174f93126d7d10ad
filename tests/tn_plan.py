"""The split plans of the TN contraction (vipant_amd/csrc/tn_plan.h: tn_plan(), tn_split_factor()) restated in plain Python, and
the case lists of tests/test_gemm_tn_gpu.py with the properties those lists must keep.

Nothing here touches a GPU.  tests/test_tn_plan_cpu.py ties the restatement to the header field by field (tests/tn_plan_main.cpp,
built by the host compiler) and to the library through the three workspace queries, and runs check_coverage() on the lists, so none
of them can drift unnoticed."""
import os
from collections import namedtuple

TP = TQ = 256            # output tile of a workgroup
BK, BK8 = 64, 128        # tokens per K-tile: bf16 kernels, e4m3 kernel
SLAB_TILE_BYTES = TP * TQ * 4
REDUCE_GRID_CAP, REDUCE_GRID_CAP_PAIR = 2048, 1024      # blocks of 256 threads x 4 floats: 32 / 16 tiles


def ceil_div(a, b):
    return -(-a // b)


def split_factor(env=None):
    """VIPANT_TN_SPLIT as the library reads it: atoi() of the variable, clamped to 1..8; unset = 1.  `env`: the variable's value
    (None: read os.environ, as the library does on every call)."""
    if env is None:
        env = os.environ.get("VIPANT_TN_SPLIT")
    if env is None:
        return 1
    s, digits = str(env).strip(), ""
    sign = -1 if s[:1] == "-" else 1
    for ch in s[1:] if s[:1] in "+-" else s:
        if not ch.isdigit():
            break
        digits += ch
    k = sign * int(digits) if digits else 0
    return 1 if k < 1 else (8 if k > 8 else k)


Launch = namedtuple("Launch", "M P Q bk tiles ntp ntq nk splits per last direct parts mtail ws_bytes slab_bytes colsum_bytes reduce_blocks cs_stride")


def _launch(M, P, Q, bk, tiles_in_plan, factor, accumulate, pair):
    ntp, ntq = ceil_div(P, TP), ceil_div(Q, TQ)
    tiles = ntp * ntq
    nk = ceil_div(M, bk)
    s = 256 // tiles_in_plan * (factor if tiles_in_plan <= 256 else 1)
    s = min(max(s, 1), nk)
    per = ceil_div(nk, s)
    splits = ceil_div(nk, per)
    last = nk - (splits - 1) * per
    slab = splits * tiles * SLAB_TILE_BYTES                                     # per problem; the workspace holds the slab(s) first,
    colsum = 0 if pair else splits * ntq * ntp * TP * 4                         # then the column-sum partials
    blocks = min(ceil_div(tiles * TP * TQ // 4, 256), REDUCE_GRID_CAP_PAIR if pair else REDUCE_GRID_CAP)
    return Launch(M, P, Q, bk, tiles, ntp, ntq, nk, splits, per, last, splits == 1 and not accumulate, splits * ntq, M % bk,
                  (2 if pair else 1) * slab + colsum, slab, colsum, blocks, ntp * TP)


def plan(M, P, Q, accumulate=False, factor=None):
    """vipant_gemm_tn.  `factor`: the VIPANT_TN_SPLIT factor (None: from the environment)."""
    tiles = ceil_div(P, TP) * ceil_div(Q, TQ)
    return _launch(M, P, Q, BK, tiles, split_factor() if factor is None else factor, accumulate, False)


def plan8(M, P, Q, accumulate=False, factor=None):
    """vipant_gemm_tn_e4m3: K-tiles of 128 tokens."""
    tiles = ceil_div(P, TP) * ceil_div(Q, TQ)
    return _launch(M, P, Q, BK8, tiles, split_factor() if factor is None else factor, accumulate, False)


def plan_pair(M, P, Q):
    """vipant_gemm_tn_pair: twice the tile count enters the plan; VIPANT_TN_SPLIT does not apply, nothing accumulates."""
    tiles = ceil_div(P, TP) * ceil_div(Q, TQ)
    return _launch(M, P, Q, BK, 2 * tiles, 1, False, True)


def splits_from_bytes(nbytes, P, Q, pair=False):
    """What a workspace query's answer says about `splits` (exact division or None)."""
    ntp, ntq = ceil_div(P, TP), ceil_div(Q, TQ)
    unit = 2 * ntp * ntq * SLAB_TILE_BYTES if pair else ntp * ntq * (SLAB_TILE_BYTES + TP * 4)
    return nbytes // unit if nbytes % unit == 0 else None


# ------------------------------------------------------------------------------------------------------------------- case lists
# (M, P, Q, layout).  layout: how the GPU tests lay the operands into their NaN-filled parents --
#   "t": tight (lda = P and ldb = Q rounded up to 8 elements, ldc = Q)
#   "p": padded leading dimensions (lda = P8 + 8, ldb = Q8 + 16, ldc = Q + 4)
#   "o": padded, and A, B and C start at a 16-byte-aligned column offset of their parents (dqkv[:, D:])
BF16_CASES = (
    [(128 * k, 2304, 2560, "tpo"[k % 3]) for k in range(1, 10)] +                 # 90 tiles, two splits of per = k
    [(833, 2048, 2048, "p"), (447, 2048, 2048, "o"), (352, 2048, 2048, "t"), (1352, 2048, 2048, "p"),   # short last splits, M tails
     (1617, 2304, 768, "o"),
     (2560, 768, 3072, "t"),                                                      # ntq = 12 > per = 6, parts = 84
     (200, 3072, 3072, "p"), (1000, 3080, 3076, "o"),                             # direct, nk = 4 / 16
     (64, 256, 256, "t"), (1, 8, 4, "t"), (63, 264, 12, "p")] +
    [(64 * n, 256, 256, "tpo"[n % 3]) for n in (2, 3, 4, 5, 8, 9)] +              # one tile: parts = splits = n
    [(385, 100, 260, "p"), (704, 776, 520, "o"), (4100, 1024, 512, "t")]
)

# the tile count entering the plan is doubled: 2 x 64 tiles leave two splits
PAIR_CASES = (
    [(128 * k, 2048, 2048, "tpo"[k % 3]) for k in (1, 3, 5, 7)] +                 # per = k
    [(256 * k, 2048, 2048, "tpo"[k % 3]) for k in range(1, 8)] +                  # per = 2 k
    [(545, 1024, 1024, "p"),                                                      # (per, last) = (2, 1), M % 64 = 33
     (129, 264, 260, "o"), (63, 264, 12, "p")]                                    # ragged: three splits of one K-tile; direct
)

# P, Q and the leading dimensions are multiples of 128 here (the scale layout's column groups)
E4M3_CASES = (
    [(256 * k, 2304, 2560, "tp"[k % 2]) for k in range(1, 8)] +                   # per = k
    [(1700, 2048, 2048, "p"),                                                     # (per, last) = (4, 2), M % 128 = 36
     (100, 128, 128, "t"), (4100, 1024, 512, "p")]                                # direct on one short K-tile; (2, 1), M % 128 = 4
)

# cases the sentinel / workspace-bound tests run on (every ragged shape of the list and one of each path), the workspace-state
# tests, and the VIPANT_TN_SPLIT tests
RAGGED_CASES = [c for c in BF16_CASES if c[1] % TP or c[2] % TQ] + [(447, 2048, 2048, "o"), (200, 3072, 3072, "p"), (64, 256, 256, "t")]
STATE_CASES = [(447, 2048, 2048, "o"), (1617, 2304, 768, "o"), (385, 100, 260, "p"), (1000, 3080, 3076, "o")]
SPLIT_ENV_CASES = [(833, 2048, 2048, "p"), (200, 3072, 3072, "p"), (640, 2304, 2560, "o")]


def case_id(c):
    return "%dx%dx%d-%s" % c


def _need(cond, what):
    assert cond, "the case list lost: " + what


def _short_pairs(ls):
    return {(l.per, l.last) for l in ls if l.splits > 1 and l.last < l.per}


def check_coverage(bf16=BF16_CASES, pair=PAIR_CASES, e4m3=E4M3_CASES):
    """What the lists must contain (VIPANT_TN_SPLIT unset).  Raises AssertionError naming the first property a list has lost."""
    ls = [plan(M, P, Q, factor=1) for M, P, Q, _ in bf16]
    lay = {(l.M, l.P, l.Q): c[3] for l, c in zip(ls, bf16)}
    assert len(set(bf16)) == len(bf16) and all(c[3] in "tpo" for c in bf16)
    pers = {l.per for l in ls}
    for k in range(1, 10):
        _need(k in pers, f"per = {k}")
    _need(any(k >= 16 for k in pers), "per >= 16")
    short = _short_pairs(ls)
    _need(len(short) >= 4, f"four (per, last) pairs with a short last split (has {sorted(short)})")
    _need(any(last == 1 for _, last in short), "a last split of one K-tile")
    _need(any((per - last) % 2 for per, last in short), "a short last split whose parity differs from per's")
    for t in (0, 1, 8, 32, 63):
        _need(any(l.mtail == t for l in ls), f"M % 64 = {t}")
    _need(any(l.direct and l.nk == 1 for l in ls), "direct with one K-tile")
    _need(any(l.direct and l.M == 1 for l in ls), "M = 1")
    _need(any(l.direct and l.nk >= 4 and l.P % TP == 0 and l.Q % TQ == 0 for l in ls), "direct, nk >= 4, whole tiles")
    _need(any(l.direct and l.nk >= 16 and l.P % TP and l.Q % TQ for l in ls), "direct, nk >= 16, ragged P and Q")
    _need(any(not l.direct and l.tiles * TP * TQ // 4 > REDUCE_GRID_CAP * 256 for l in ls), "a slab launch over the reduce grid's cap")
    parts = {l.parts for l in ls}
    for n in (1, 2, 3, 4, 5, 8, 9, 12, 13):
        _need(n in parts, f"parts = {n}")
    _need(any(n > 32 for n in parts), "parts > 32")
    _need(any(l.ntq > l.per for l in ls), "ntq > per")
    _need(any(l.P % 8 and lay[(l.M, l.P, l.Q)] in "po" for l in ls), "P % 8 != 0 under a padded lda")
    _need(any(l.Q == 4 and lay[(l.M, l.P, l.Q)] == "t" for l in ls), "Q = 4 under ldb = 8")
    _need(any(l.P == 264 for l in ls) and any(l.Q == 260 for l in ls), "P = 264 and Q = 260")
    for tag in "tpo":
        _need(sum(c[3] == tag for c in bf16) >= 5, f"layout {tag!r}")
    _need(all(M <= 4100 for M, _, _, _ in bf16), "small M")

    lp = [plan_pair(M, P, Q) for M, P, Q, _ in pair]
    le = [plan8(M, P, Q, factor=1) for M, P, Q, _ in e4m3]
    for name, lst in (("pair", lp), ("e4m3", le)):
        for k in range(1, 8):
            _need(any(l.per == k for l in lst), f"{name}: per = {k}")
        _need(_short_pairs(lst), f"{name}: a short last split")
        _need(any(l.mtail for l in lst), f"{name}: an M tail")
        _need(any(l.direct for l in lst) and any(not l.direct for l in lst), f"{name}: both store paths")
    _need(any(not l.direct and l.tiles * TP * TQ // 4 > REDUCE_GRID_CAP_PAIR * 256 for l in lp), "pair: more than 16 tiles")
    _need(any(l.P % TP and l.Q % TQ for l in lp), "pair: ragged P and Q")
    _need(all(P % 128 == 0 and Q % 128 == 0 and lay_ in "tp" for _, P, Q, lay_ in e4m3), "e4m3: multiples of 128")
    for c in RAGGED_CASES + STATE_CASES:
        _need(c in bf16, f"{c} (named by a sub-list)")
    for M, P, Q, _ in SPLIT_ENV_CASES:
        _need(any(c[:3] == (M, P, Q) for c in bf16), f"{(M, P, Q)} (VIPANT_TN_SPLIT tests)")
        _need(len({(plan(M, P, Q, factor=f).splits, plan(M, P, Q, factor=f).per) for f in (1, 2, 4)}) == 3,
              f"{(M, P, Q)}: three different plans under VIPANT_TN_SPLIT = 1, 2, 4")


# ------------------------------------------------------------------------------------------------------------------- error depths
def depth_c(l, accumulate):
    """Longest chain of fp32 additions one product of C passes through (derivation: tests/test_gemm_tn_gpu.py)."""
    return 32 + (l.bk // 32) * l.per + l.splits + (1 if accumulate else 0)


def depth_colsum(l, accumulate):
    """The same for one element of A on its way into a_colsum (bf16 kernel)."""
    turns = ceil_div(l.per, l.ntq)
    return 4 * turns + 16 + (ceil_div(l.parts, 8) + 1) + 1 + 2 + (1 if accumulate else 0)
