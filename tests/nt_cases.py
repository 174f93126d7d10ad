"""The case lists of tests/test_gemm_nt_gpu.py -- one record per launch of vipant_gemm_nt / vipant_gemm_nt_e4m3 with the kernel instance
that launch must reach -- and what the three NT parity files share: the layout arithmetic, the error budgets, the restated queue
lengths of the ticket walk and the line format of the selector driver (tests/nt_select_main.cpp).

Nothing here touches a GPU or imports torch.  tests/test_nt_cases_cpu.py feeds every case to the selector driver, parses the instance
lists out of vipant_amd/csrc/gemm_nt.hip and runs check_coverage(), so that neither the lists nor the library can drift unnoticed."""
from collections import namedtuple

TILE, BK = 256, 64
# VIPANT_EPI_* (include/vipant_hip.h)
BF16, F32, RESIDUAL_F32, QUICKGELU, DQUICKGELU, SCALE_F32, QUICKGELU_D8, DQUICKGELU_D8 = range(8)
# VIPANT_SW_* (vipant_amd/csrc/switches.h); test_nt_cases_cpu.py compares the values with the header
SW = {"GA": 1 << 11, "GN": 1 << 12, "E4M3_KSTEP": 1 << 15, "DA": 1 << 17, "DN": 1 << 18, "SW": 1 << 22, "R4": 1 << 23,
      "E4M3_EMIT_PLAIN_WALK": 1 << 25, "E4M3_WIDE_PLAIN_WALK": 1 << 26}
SW_HEADER_NAMES = {"GA": "GROUPED_ALWAYS", "GN": "GROUPED_NEVER", "E4M3_KSTEP": "E4M3_KSTEP", "DA": "DEEP_ALWAYS", "DN": "DEEP_NEVER",
                   "SW": "STATIC_WALK", "R4": "ROUND4_SCHEDULES", "E4M3_EMIT_PLAIN_WALK": "E4M3_EMIT_PLAIN_WALK",
                   "E4M3_WIDE_PLAIN_WALK": "E4M3_WIDE_PLAIN_WALK"}
GA, DA, DN, R4, STATIC = SW["GA"], SW["DA"], SW["DN"], SW["R4"], SW["SW"]
KSTEP, KSTEP_GROUPED, DEEP, DEEP_GROUPED = 0, 8, 10, 12            # NtSchedule
EMIT_NONE, EMIT_ALSO, EMIT_ALONE, EMIT_WITH_CODES = range(4)        # NtEmit

# kind: "bf16" | "e4m3".  lay: "t" tight, "p" padded (lda, ldb > K, ldc > N), "o" offset by a 16-byte-aligned column inside a padded
# parent.  ldc: 0 = what the layout gives, else this row length of C and aux (column offset 0).  inplace: RESIDUAL_F32 with aux == C.
Case = namedtuple("Case", "kind M N K epi few sw c_null aux_null cq_null lay ldc inplace inst")


def ceil_div(a, b):
    return -(-a // b)


def pp(epi, sched, es=2, emit=0, ticket=0):
    return f"pingpong epi={epi} sched={sched} es={es} emit={emit} ticket={ticket}"


def plain(epi):
    return f"plain epi={epi}"


def few_rows(epi):
    return f"few_rows epi={epi}"


def bf16_case(M, N, K, epi, inst, sw=0, lay="t", ldc=0, few=False, inplace=False):
    aux_null = epi in (BF16, F32, SCALE_F32)
    return Case("bf16", M, N, K, epi, few, sw, False, aux_null, True, lay, ldc, inplace, inst)


def e4m3_case(M, N, K, epi, emit, sched, sw=0, lay="t"):
    """The NULL arguments that select an emit mode (nt_select_e4m3): NONE: no cq; ALSO: C, aux and cq; ALONE: cq without C (QuickGELU:
    without aux too; QuickGELU': aux is the input); WITH_CODES: cq and aux without C."""
    c_null = emit in (EMIT_ALONE, EMIT_WITH_CODES)
    aux_null = epi == BF16 or (epi == QUICKGELU_D8 and emit == EMIT_ALONE)
    return Case("e4m3", M, N, K, epi, False, sw, c_null, aux_null, emit == EMIT_NONE, lay, 0, False, pp(epi, sched, 1, emit, 0))


def case_id(c):
    sw = "+".join(k for k, v in SW.items() if c.sw & v) or "0"
    extra = (",ldc%d" % c.ldc if c.ldc else "") + (",inplace" if c.inplace else "") + (",few" if c.few else "")
    nul = "".join(n for n, f in (("C", c.c_null), ("a", c.aux_null), ("q", c.cq_null)) if not f)
    return f"{c.kind}-{c.M}x{c.N}x{c.K}-e{c.epi}-{sw}-{c.lay}{extra}-{nul}"


# ------------------------------------------------------------------------------------------------------------------- layout
def layout(c):
    """(lda, ldb, ldc, column offsets of A, B and C) in elements.  bf16 operands need lda, ldb % 8 == 0 and 16-byte-aligned pointers;
    the offset of C is also the BYTE offset of a code matrix, hence 16.  Padding keeps ldc's remainder modulo 16 (the QUICKGELU_D8
    store paths).  e4m3 operands stay contiguous (lda = ldb = K: the scale layout is tied to the row length); C and aux are padded."""
    if c.ldc:
        ldc, oc = c.ldc, 0
    elif c.lay == "t":
        ldc, oc = c.N, 0
    elif c.lay == "p":
        ldc, oc = c.N + 16, 0
    else:
        ldc, oc = c.N + 48, 16
    if c.kind == "e4m3" or c.lay == "t":
        return c.K, c.K, ldc, 0, 0, oc
    if c.lay == "p":
        return c.K + 8, c.K + 24, ldc, 0, 0, oc
    return c.K + 40, c.K + 16, ldc, 24, 8, oc


def driver_line(c):
    """One line of stdin of tests/nt_select_main.cpp: kind M N K ldc epilogue few_rows C_null aux_null cq_null aux_misaligned switches."""
    return "%s %d %d %d %d %d %d %d %d %d 0 %d" % (c.kind, c.M, c.N, c.K, layout(c)[2], c.epi, int(c.few), int(c.c_null), int(c.aux_null),
                                                  int(c.cq_null), c.sw)


def parse_instance(s):
    """A line of the driver's stdout -> (family, epilogue, schedule, es, emit, ticket); the last four None outside the ping-pong family."""
    f = s.split()
    kv = dict(x.split("=") for x in f[1:])
    if f[0] == "pingpong":
        return ("pingpong", int(kv["epi"]), int(kv["sched"]), int(kv["es"]), int(kv["emit"]), int(kv["ticket"]))
    return (f[0], int(kv["epi"]), None, None, None, None)


# ------------------------------------------------------------------------------------------------------------------- ticket walk
def queue_lengths(c):
    """qlen_own of gemm_nt_pp_kernel for the eight queues (one per XCD) of a full-grid launch on the case's schedule."""
    sched = parse_instance(c.inst)[2]
    ntm, ntn = ceil_div(c.M, TILE), ceil_div(c.N, TILE)
    out = []
    for xq in range(8):
        if sched in (KSTEP_GROUPED, DEEP_GROUPED):
            cg, ppx = ntn // 2, (ntm + 3) // 4
            rows = min(max(ntm - (xq & 3) * ppx, 0), ppx)
            out.append(rows * cg)
        else:
            tiles = ntm * ntn
            rem = min(max((tiles & 255) - xq * 32, 0), 32)
            out.append((tiles >> 8) * 32 + rem)
    return out


def draws(c):
    """(positions per draw at the start, taper): DRAW2 epilogues draw pairs throughout; BF16 launches with >= 8 column tiles draw pairs
    and single positions for the last 96 of a queue; everything else single positions."""
    epi = parse_instance(c.inst)[1]
    if epi in (QUICKGELU_D8, DQUICKGELU_D8):
        return 2, False
    return (2 if epi == BF16 and ceil_div(c.N, TILE) >= 8 else 1), True


def queue_classes(c):
    """The queue-length classes a ticket launch belongs to (the issue's list)."""
    q = queue_lengths(c)
    n, taper = draws(c)
    grouped = parse_instance(c.inst)[2] in (KSTEP_GROUPED, DEEP_GROUPED)
    out = set()
    if n == 2 and not taper and any(x & 1 for x in q):
        out.add("odd pairs, grouped walk" if grouped else "odd pairs, plain walk")
    if not grouped and len(set(q)) > 1 and 225 <= ((ceil_div(c.M, TILE) * ceil_div(c.N, TILE)) & 255) <= 255:
        out.add("unequal queues")
    if grouped and q[3] < q[0]:
        out.add("short last quarter")
    if n == 2 and taper:
        # the first draw is taken with tk_n = 2 whatever the length; the taper applies from 128 + drawn + 96 >= qlen on
        out.add("pairs, then the taper" if max(q) > 224 else "taper only")
        if not grouped and max(q) > 224:
            out.add("plain walk, pairs in front of the taper")
    if n == 1:
        out.add("single draws")
    return out


# ------------------------------------------------------------------------------------------------------------------- the lists
LAYS = "tpo"


def _ticket_cases():
    table = [  # M, N, epilogue, switches, schedule
        (109300, 768, BF16, 0, KSTEP), (109300, 768, QUICKGELU, 0, KSTEP), (109300, 768, QUICKGELU_D8, 0, KSTEP),
        (109300, 768, DQUICKGELU, DN, KSTEP), (109300, 768, DQUICKGELU_D8, DN, KSTEP),
        (65300, 1280, BF16, 0, DEEP),
        (26800, 3072, QUICKGELU, DA, DEEP), (26800, 3072, DQUICKGELU, DA, DEEP), (26800, 3072, QUICKGELU_D8, DA, DEEP),
        (26800, 3072, DQUICKGELU_D8, DA, DEEP),
        (132000, 512, BF16, GA, KSTEP_GROUPED), (132000, 512, QUICKGELU, GA, KSTEP_GROUPED), (132000, 512, DQUICKGELU, GA, KSTEP_GROUPED),
        (132000, 512, DQUICKGELU_D8, GA, KSTEP_GROUPED), (132000, 512, QUICKGELU_D8, R4, KSTEP_GROUPED),
        (132000, 512, QUICKGELU_D8, 0, DEEP_GROUPED), (132000, 512, DQUICKGELU_D8, 0, DEEP_GROUPED),
        (22400, 3072, QUICKGELU_D8, 0, DEEP_GROUPED), (22400, 3072, DQUICKGELU_D8, 0, DEEP_GROUPED),
        (33700, 2048, BF16, 0, DEEP_GROUPED),        # queues of 132: taper only
        (58300, 2048, BF16, 0, DEEP_GROUPED),        # queues of 228: pairs, then the taper
        # queue-length classes on top of the table
        (108600, 768, BF16, 0, KSTEP),               # 1275 tiles: queues of 160 (seven) and 155
        (108600, 768, DQUICKGELU_D8, DN, KSTEP),     # pairs out of those queues, one of them odd
        (67228, 1024, QUICKGELU_D8, 0, DEEP_GROUPED),  # 263 row tiles: quarters of 66, 66, 66, 65 row tiles, queues of 132 and 130
        (51200, 2304, BF16, 0, DEEP),                # 1800 tiles, nine column tiles: queues of 232 and 224, pairs in front of the taper
    ]
    out = []
    for i, (M, N, epi, sw, sched) in enumerate(table):
        lay = LAYS[i % 3]
        out.append(bf16_case(M, N, 256, epi, pp(epi, sched, ticket=1), sw=sw, lay=lay))
        out.append(bf16_case(M, N, 256, epi, pp(epi, sched, ticket=0), sw=sw | STATIC, lay=lay))
    return out


TICKET_CASES = _ticket_cases()        # pairs: [2 i] on tickets, [2 i + 1] its static twin

# what test_ticket_walk launches between two ticket launches of a case: a ticket launch of another shape
TICKET_NEIGHBOURS = [bf16_case(66000, 1280, 256, BF16, pp(BF16, DEEP, ticket=1)), TICKET_CASES[0]]

K_TILE_SWEEP = (128, 192, 256, 320, 384, 448, 512, 576, 1024)


def _static_cases():
    out = []
    # 33000 x 512 = 129 x 2 = 258 tiles: the K-tile stream wraps from tile to tile; two to nine and sixteen K-tiles per schedule
    for i, K in enumerate(K_TILE_SWEEP):
        lay = LAYS[i % 3]
        out.append(bf16_case(33000, 512, K, BF16, pp(BF16, KSTEP), sw=DN if K >= 1024 else 0, lay=lay))
        out.append(bf16_case(33000, 512, K, BF16, pp(BF16, KSTEP_GROUPED), sw=GA, lay=lay))
        out.append(bf16_case(33000, 512, K, BF16, pp(BF16, DEEP), sw=DA, lay=lay))
        out.append(bf16_case(33000, 512, K, QUICKGELU_D8, pp(QUICKGELU_D8, DEEP_GROUPED), lay=lay))
    # the grouped walk with every remainder of the row-tile count modulo 4 (129 row tiles above; 130, 131, 128 here)
    for M in (33100, 33400, 32700):
        out.append(bf16_case(M, 512, 128, QUICKGELU_D8, pp(QUICKGELU_D8, DEEP_GROUPED), lay="p"))
        out.append(bf16_case(M, 512, 128, BF16, pp(BF16, KSTEP_GROUPED), sw=GA, lay="o"))
    # a second column tile of 8 columns and the 8-column store path of QUICKGELU_D8; the 16-column path and its fallback
    for N, ldc in ((264, 264), (264, 272), (512, 512), (512, 520)):
        out.append(bf16_case(33000, N, 128, QUICKGELU_D8, pp(QUICKGELU_D8, DEEP_GROUPED), ldc=ldc))
        out.append(bf16_case(33000, N, 192, DQUICKGELU_D8, pp(DQUICKGELU_D8, DEEP_GROUPED), ldc=ldc))
    out.append(bf16_case(33000, 264, 128, BF16, pp(BF16, KSTEP), ldc=272))
    # eight column tiles, the eighth of 8 columns: BF16 on DEEP_GROUPED
    out.append(bf16_case(7990, 1800, 128, BF16, pp(BF16, DEEP_GROUPED), lay="p"))
    return out


STATIC_CASES = _static_cases()

PP_EPILOGUES = (BF16, QUICKGELU, DQUICKGELU, QUICKGELU_D8, DQUICKGELU_D8)


def _small_cases():
    """Fewer than 256 tiles: one to three tiles and nine (the grid is rounded up to 16), every bf16 ping-pong epilogue."""
    shapes = [(1, 8, 128), (127, 248, 192), (128, 256, 256), (129, 264, 128), (255, 264, 192), (257, 256, 320), (600, 248, 128),
              (700, 768, 192), (257, 264, 1024)]
    out = []
    for i, (M, N, K) in enumerate(shapes):
        for epi in PP_EPILOGUES:
            # nt_schedule_bf16 without switches: QuickGELU' from the codes and BF16 with K >= 1024 run DEEP
            sched = DEEP if epi == DQUICKGELU_D8 or (epi == BF16 and K >= 1024) else KSTEP
            out.append(bf16_case(M, N, K, epi, pp(epi, sched), lay=LAYS[(i + epi) % 3]))
    return out


SMALL_CASES = _small_cases()

PLAIN_EPILOGUES = (BF16, F32, RESIDUAL_F32, QUICKGELU, DQUICKGELU, SCALE_F32)


def _plain_cases():
    out = []
    for i, epi in enumerate(PLAIN_EPILOGUES):
        fp32 = epi in (F32, RESIDUAL_F32, SCALE_F32)
        out.append(bf16_case(300, 264, 64, epi, plain(epi), lay=LAYS[i % 3]))                  # K = 64
        out.append(bf16_case(129, 4, 128, epi, plain(epi), lay="t"))                            # N % 8 == 4
        out.append(bf16_case(515, 260, 192, epi, plain(epi), lay=LAYS[(i + 1) % 3]))
        out.append(bf16_case(257, 256, 128, epi, plain(epi), ldc=260))                          # ldc % 8 == 4
        if fp32:
            out.append(bf16_case(260, 520, 1024, epi, plain(epi), lay=LAYS[(i + 2) % 3]))       # staged shapes stay here for fp32 outputs
    out.append(bf16_case(300, 264, 64, RESIDUAL_F32, plain(RESIDUAL_F32), lay="p", inplace=True))
    out.append(bf16_case(260, 520, 1024, RESIDUAL_F32, plain(RESIDUAL_F32), lay="o", inplace=True))
    return out


PLAIN_CASES = _plain_cases()

FEW_ROWS_EPILOGUES = (BF16, F32, RESIDUAL_F32, QUICKGELU_D8, DQUICKGELU_D8)
FEW_ROWS_K = (64, 192, 256, 768, 832, 1600)      # six 32-deep K-steps per wave and batch, four waves: period 768; 64 leaves three waves idle
FEW_ROWS_MN = ((1, 4), (63, 60), (64, 64), (65, 68), (130, 520))


def _few_rows_cases():
    out = []
    for i, (M, N) in enumerate(FEW_ROWS_MN):
        for j, K in enumerate(FEW_ROWS_K):
            for epi in FEW_ROWS_EPILOGUES:
                out.append(bf16_case(M, N, K, epi, few_rows(epi), lay=LAYS[(i + j) % 3], few=True))
    out.append(bf16_case(130, 520, 832, RESIDUAL_F32, few_rows(RESIDUAL_F32), lay="p", few=True, inplace=True))
    return out


FEW_ROWS_CASES = _few_rows_cases()

E4M3_EMIT_MODES = ((QUICKGELU_D8, EMIT_NONE), (QUICKGELU_D8, EMIT_ALSO), (QUICKGELU_D8, EMIT_ALONE), (QUICKGELU_D8, EMIT_WITH_CODES),
                   (DQUICKGELU_D8, EMIT_NONE), (DQUICKGELU_D8, EMIT_ALSO), (DQUICKGELU_D8, EMIT_ALONE))


def _e4m3_cases():
    out = []
    for K in (256, 768):
        lay = "p" if K == 256 else "o"
        # 700 x 512: the nine ungrouped instances
        out.append(e4m3_case(700, 512, K, BF16, EMIT_NONE, DEEP, lay=lay))
        out.append(e4m3_case(700, 512, K, BF16, EMIT_NONE, KSTEP, sw=SW["E4M3_KSTEP"], lay=lay))
        for epi, emit in E4M3_EMIT_MODES:
            out.append(e4m3_case(700, 512, K, epi, emit, KSTEP, lay=lay))
        # 32600 x 512 = 128 x 2 tiles, M % 32 = 24: the four grouped emit instances, ALONE with QUICKGELU_D8 (it stays on the plain walk),
        # and every one of them again on the plain walk
        for epi, emit in E4M3_EMIT_MODES:
            grouped = emit != EMIT_NONE and not (epi == QUICKGELU_D8 and emit == EMIT_ALONE)
            out.append(e4m3_case(32600, 512, K, epi, emit, KSTEP_GROUPED if grouped else KSTEP, lay=lay))
            if grouped:
                out.append(e4m3_case(32600, 512, K, epi, emit, KSTEP, sw=SW["E4M3_EMIT_PLAIN_WALK"], lay=lay))
        out.append(e4m3_case(7990, 2048, K, BF16, EMIT_NONE, DEEP_GROUPED, lay=lay))
        out.append(e4m3_case(7990, 2048, K, BF16, EMIT_NONE, DEEP, sw=SW["E4M3_WIDE_PLAIN_WALK"], lay=lay))
        out.append(e4m3_case(7990, 1024, K, BF16, EMIT_NONE, DEEP, lay=lay))
        out.append(e4m3_case(7990, 1024, K, BF16, EMIT_NONE, KSTEP, sw=SW["E4M3_KSTEP"], lay=lay))
    return out


E4M3_CASES = _e4m3_cases()

# refusals (part e): (case, what the selector driver prints)
REFUSALS = [
    (bf16_case(300, 256, 64, QUICKGELU_D8, "refuse D8_NEEDS_STAGED"), "the D8 epilogues at K = 64"),
    (bf16_case(300, 256, 64, DQUICKGELU_D8, "refuse D8_NEEDS_STAGED"), "the D8 epilogues at K = 64"),
    (bf16_case(300, 260, 128, QUICKGELU_D8, "refuse D8_NEEDS_STAGED"), "D8 with N % 8 = 4"),
    (bf16_case(300, 260, 128, DQUICKGELU_D8, "refuse D8_NEEDS_STAGED"), "D8 with N % 8 = 4"),
    (bf16_case(64, 64, 256, SCALE_F32, "refuse FEW_ROWS_EPILOGUE", few=True), "a few-rows launch with SCALE_F32"),
]
# a misaligned aux is a property of the pointer, not of the case: (the case with the instance it reaches when aux is aligned, what the
# selector driver prints with aux_misaligned = 1, why)
MISALIGNED_AUX = [
    (bf16_case(300, 256, 128, QUICKGELU_D8, pp(QUICKGELU_D8, KSTEP)), "refuse D8_NEEDS_STAGED", "D8 with a misaligned aux"),
    (bf16_case(300, 256, 128, DQUICKGELU_D8, pp(DQUICKGELU_D8, DEEP)), "refuse D8_NEEDS_STAGED", "D8 with a misaligned aux"),
    (bf16_case(64, 64, 256, QUICKGELU_D8, few_rows(QUICKGELU_D8), few=True), "refuse D8_NEEDS_ALIGNED_AUX", "few-rows D8 with a misaligned aux"),
]

ALL_CASES = TICKET_CASES + TICKET_NEIGHBOURS[:1] + STATIC_CASES + SMALL_CASES + PLAIN_CASES + FEW_ROWS_CASES + E4M3_CASES


# ------------------------------------------------------------------------------------------------------------------- budgets
U32 = 2.0 ** -23          # one fp32 addition; 2^-23 rather than 2^-24 because the matrix unit's adder may truncate
U16 = 2.0 ** -8           # one rounding to bf16 (eight significant bits)
GATE = 64 * U32           # the gate's fp32 arithmetic: v_exp_f32 and v_rcp_f32 at about one ulp each, the argument's rounding amplified by
                          # |1.702 u| <= 40 (20 x 2^-23), the sum, the product: under 32 x 2^-23, with a margin of two
CODE_SLACK = 0.5 + 0.01   # rounding to the nearest code + the same arithmetic in code units (212.5 x 1.1 x 32 x 2^-23 = 9e-4), margin six and more
DECODE = 4 * 2.0 ** -24   # gelu_decode in fp32: the constant 1 / 212.5, the product, the constant 0.1, the difference -- absolute, values <= 1.2
FLUSH = 2.0 ** -126       # fp32 results below the normal range are flushed to zero by v_exp_f32 / v_rcp_f32
LIP_G, LIP_CODE = 1.1, 0.851        # |QuickGELU'| <= 1.1, |QuickGELU''| <= 0.851 (1.702 / 2)


def depth(c):
    """The longest chain of additions one product passes through, read from the kernels: the 32 products of one
    v_mfma_f32_16x16x32_bf16, K / 32 accumulator steps, the bias; the few-rows kernel adds its four waves' partial tiles (3); a
    residual (1); SCALE_F32's multiplication by alpha counts as one more rounding."""
    fam = parse_instance(c.inst)[0]
    return 32 + c.K // 32 + 1 + (3 if fam == "few_rows" else 0) + (1 if c.epi == RESIDUAL_F32 else 0) + (1 if c.epi == SCALE_F32 else 0)


# ------------------------------------------------------------------------------------------------------------------- coverage
def _need(ok, what):
    assert ok, "lost: " + what


def check_coverage(ticket=None, static=None, small=None, plain_=None, few=None, e4m3=None):
    """What the lists were chosen for (the issue's list).  AssertionError("lost: ...") names what a dropped case took with it."""
    ticket = TICKET_CASES if ticket is None else ticket
    static = STATIC_CASES if static is None else static
    small = SMALL_CASES if small is None else small
    plain_ = PLAIN_CASES if plain_ is None else plain_
    few = FEW_ROWS_CASES if few is None else few
    e4m3 = E4M3_CASES if e4m3 is None else e4m3
    inst = lambda c: parse_instance(c.inst)
    # ticket walk: every launch has its static twin at the same shape, and every queue-length class is met
    on = [c for c in ticket if inst(c)[5] == 1]
    twins = {(c.M, c.N, c.K, c.epi, c.sw & ~STATIC, c.lay) for c in ticket if inst(c)[5] == 0 and c.sw & STATIC}
    for c in on:
        _need((c.M, c.N, c.K, c.epi, c.sw, c.lay) in twins, f"the static twin of {case_id(c)}")
        _need(min(queue_lengths(c)) > 128 and c.K >= 256, f"{case_id(c)} draws tickets")
    classes = set().union(*[queue_classes(c) for c in on]) if on else set()
    for want in ("odd pairs, plain walk", "odd pairs, grouped walk", "unequal queues", "short last quarter", "taper only",
                 "pairs, then the taper", "plain walk, pairs in front of the taper", "single draws"):
        _need(want in classes, f"ticket walk queue class `{want}`")
    _need(any(c.epi == BF16 and max(queue_lengths(c)) == 132 for c in on) and any(c.epi == BF16 and max(queue_lengths(c)) == 228 for c in on),
          "the BF16 launches with queues of 132 and of 228")
    # static walk over more than 256 tiles: the K-tile counts per schedule
    big = [c for c in static if ceil_div(c.M, TILE) * ceil_div(c.N, TILE) > 256]
    for sched in (KSTEP, KSTEP_GROUPED, DEEP, DEEP_GROUPED):
        got = {c.K // BK for c in big if inst(c)[2] == sched}
        _need(got >= {k // BK for k in K_TILE_SWEEP}, f"K-tile counts {sorted({k // BK for k in K_TILE_SWEEP} - got)} on schedule {sched}, static walk over 258 tiles")
    for sched in (KSTEP_GROUPED, DEEP_GROUPED):
        got = {ceil_div(c.M, TILE) % 4 for c in static if inst(c)[2] == sched and ceil_div(c.M, TILE) * ceil_div(c.N, TILE) >= 256}
        _need(got == {0, 1, 2, 3}, f"row-tile count modulo 4 = {sorted({0, 1, 2, 3} - got)} on the grouped schedule {sched}")
    # both store paths of QUICKGELU_D8, chosen on purpose: 16 columns per thread needs N % 16 == 0 and ldc % 16 == 0
    d8 = [(c.N % 16 == 0, layout(c)[2] % 16 == 0) for c in static + ticket + small if c.epi == QUICKGELU_D8]
    for want, what in (((True, True), "16-column path"), ((True, False), "fallback for ldc % 16 != 0"), ((False, False), "N % 16 == 8, ldc % 16 == 8"),
                       ((False, True), "N % 16 == 8, ldc % 16 == 0")):
        _need(want in d8, f"QUICKGELU_D8 store path: {what}")
    _need(any(c.M == 7990 and c.N == 1800 and inst(c)[1:3] == (BF16, DEEP_GROUPED) for c in static), "BF16 on DEEP_GROUPED with a ragged eighth column tile")
    # fewer than 256 tiles
    for epi in PP_EPILOGUES:
        mine = [c for c in small if c.epi == epi]
        tiles = {ceil_div(c.M, TILE) * ceil_div(c.N, TILE) for c in mine}
        _need(tiles >= {1, 2, 3, 9}, f"tile counts {sorted({1, 2, 3, 9} - tiles)} of epilogue {epi}")
        _need({c.M for c in mine} >= {1, 127, 128, 129, 255, 257}, f"M remainders of epilogue {epi}")
        _need({c.N for c in mine} >= {8, 248, 256, 264}, f"N remainders of epilogue {epi}")
    # plain kernel
    for epi in PLAIN_EPILOGUES:
        mine = [c for c in plain_ if c.epi == epi]
        _need(any(c.K == 64 for c in mine), f"plain epilogue {epi} at K = 64")
        _need({c.N for c in mine} >= {4, 260}, f"plain epilogue {epi} with N % 8 == 4")
        _need(any(layout(c)[2] % 8 == 4 and c.N % 8 == 0 for c in mine), f"plain epilogue {epi} with ldc % 8 == 4")
        if epi in (F32, RESIDUAL_F32, SCALE_F32):
            _need(any(c.K == 1024 for c in mine), f"plain fp32 epilogue {epi} at K = 1024")
    _need({c.inplace for c in plain_ if c.epi == RESIDUAL_F32} == {False, True}, "RESIDUAL_F32 in place and not in place")
    # few-rows kernel
    for epi in FEW_ROWS_EPILOGUES:
        mine = [c for c in few if c.epi == epi]
        _need({c.K for c in mine} >= set(FEW_ROWS_K), f"few-rows epilogue {epi}: K")
        _need({c.M for c in mine} >= {1, 63, 64, 65, 130} and {c.N for c in mine} >= {4, 60, 64, 68, 520}, f"few-rows epilogue {epi}: M and N")
    # e4m3
    for K in (256, 768):
        mine = [c for c in e4m3 if c.K == K]
        _need(len({c.inst for c in mine if (c.M, c.N) == (700, 512)}) == 9, f"the nine ungrouped e4m3 instances at K = {K}")
        g = {c.inst for c in mine if (c.M, c.N) == (32600, 512) and inst(c)[2] == KSTEP_GROUPED}
        _need(len(g) == 4, f"the four grouped emit instances at K = {K}")
        _need(any((c.M, c.N) == (32600, 512) and inst(c)[1:5] == (QUICKGELU_D8, KSTEP, 1, EMIT_ALONE) for c in mine), f"ALONE with QUICKGELU_D8 at 256 tiles, K = {K}")
        _need(any(c.sw & SW["E4M3_EMIT_PLAIN_WALK"] for c in mine) and any(c.sw & SW["E4M3_WIDE_PLAIN_WALK"] for c in mine), f"plain-walk twins at K = {K}")
        _need({inst(c)[2] for c in mine if (c.M, c.N, c.epi) == (7990, 1024, BF16)} == {DEEP, KSTEP} and
              {inst(c)[2] for c in mine if (c.M, c.N, c.epi) == (7990, 2048, BF16)} == {DEEP_GROUPED, DEEP}, f"the e4m3 BF16 schedules at K = {K}")
    _need(any(c.M % 32 != 0 and c.M % 128 != 0 and not c.cq_null for c in e4m3), "an emitted form with a ragged last row panel")
    _need(all(layout(c)[0] == c.K and layout(c)[1] == c.K for c in e4m3) and all(layout(c)[2] > c.N and layout(c)[2] % 8 == 0 for c in e4m3), "e4m3: contiguous operands, ldc > N with ldc % 8 == 0")
    # M and N remainders over everything that runs the 256 x 256 kernels
    every = ticket + static + small
    _need({c.M % TILE for c in every} >= {0, 1, 127, 128, 129, 255}, "M remainders modulo the tile")
    _need({c.N % TILE for c in every} >= {0, 8, 248}, "N remainders modulo the tile")
    _need({c.lay for c in every} == set(LAYS) and {c.lay for c in few} == set(LAYS) and {c.lay for c in plain_} == set(LAYS), "the three layouts")
