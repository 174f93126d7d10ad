// Which kernel instance of gemm_nt.hip a launch reaches: pure functions of the launch's shape, epilogue, NULL arguments and the
// VIPANT_GEMM_VARIANT switches.  Host-only header (nothing from HIP): tests/test_nt_select_cpu.py compiles it alone and checks it
// against a recorded table.  The measurements that justify a rule stand beside the rule; gemm_nt.hip maps the result to a template
// instance (NT_PP_INSTANCES there lists every ping-pong instance the library holds).
#pragma once
#include <stdint.h>

#include "../../include/vipant_hip.h"
#include "switches.h"

enum NtFamily { NT_PLAIN, NT_PINGPONG, NT_FEW_ROWS };      // one 256 x 256 tile per workgroup | persistent ping-pong | 64 x 64 tiles, K split over waves
// schedules of the ping-pong kernel (the values are its VAR template argument)
enum NtSchedule {
    NT_KSTEP = 0,             // barrier intervals by k-step
    NT_KSTEP_GROUPED = 8,     // the same on the column-grouped tile walk
    NT_DEEP = 10,             // three intervals of look-ahead for every operand piece, intervals by row halves
    NT_DEEP_GROUPED = 12,     // DEEP on the column-grouped walk
};
// what a ping-pong epilogue leaves (the values are the kernel's EMIT template argument; e4m3 operands only beyond NT_EMIT_NONE)
enum NtEmit {
    NT_EMIT_NONE = 0,         // the bf16 result only
    NT_EMIT_ALSO = 1,         // the bf16 result (and codes) and its e4m3 form
    NT_EMIT_ALONE = 2,        // the e4m3 form alone
    NT_EMIT_WITH_CODES = 3,   // the e4m3 form and the QuickGELU' codes, no bf16 result
};
struct NtInstance {
    NtFamily family;
    int epilogue;             // VIPANT_EPI_* without VIPANT_EPI_FEW_ROWS
    NtSchedule schedule;      // ping-pong only
    int es;                   // bytes per operand element: 2 = bf16, 1 = e4m3
    NtEmit emit;
    bool ticket;              // ping-pong only: the ticket walk (else the static stride)
};
// why a launch is refused (the entry points of gemm_nt.hip hold the messages; all are VIPANT_EBADSHAPE)
enum NtRefusal {
    NT_ACCEPT = 0,
    NT_UNKNOWN_EPILOGUE,
    NT_FEW_ROWS_EPILOGUE,     // VIPANT_EPI_FEW_ROWS with an epilogue the few-rows kernel does not have
    NT_RESIDUAL_NEEDS_AUX,
    NT_QUICKGELU_NEEDS_AUX,
    NT_DQUICKGELU_NEEDS_AUX,
    NT_D8_NEEDS_AUX,
    NT_D8_NEEDS_ALIGNED_AUX,  // few-rows and e4m3 launches: aux missing or not 16-byte aligned
    NT_D8_NEEDS_STAGED,       // N % 8, ldc % 8, K >= 128 or the alignment of aux
    NT_E4M3_C_WITHOUT_AUX,
};
struct NtLaunch {
    int64_t M, N, K, ldc;
    int epilogue;             // VIPANT_EPI_* without VIPANT_EPI_FEW_ROWS
    bool few_rows;            // VIPANT_EPI_FEW_ROWS was set
    bool c_null, aux_null, cq_null;
    bool aux_misaligned;      // aux is not 16-byte aligned
    int switches;             // vipant_switches()
};

constexpr int64_t NT_TILE = 256, NT_BK = 64;       // BM = BN and BK of nt_core.h

static inline int64_t nt_row_tiles(const NtLaunch& l) { return (l.M + NT_TILE - 1) / NT_TILE; }
static inline int64_t nt_col_tiles(const NtLaunch& l) { return (l.N + NT_TILE - 1) / NT_TILE; }

// the column-grouped walk (the XCDs split into two column groups times four row quarters) needs the full grid of 256 and an even
// number of column tiles
static inline bool nt_groupable(const NtLaunch& l) {
    return nt_col_tiles(l) % 2 == 0 && nt_row_tiles(l) * nt_col_tiles(l) >= 256;
}
static inline bool nt_grouped(NtSchedule s) { return s == NT_KSTEP_GROUPED || s == NT_DEEP_GROUPED; }

// ticket walk (common.h) when every XCD's queue holds more than the three rounds a workgroup takes statically: the shortest queue
// of the plain walk is the last one, of the column-grouped walk the one of the last row quarter.  It exists for the bf16 kernels
// (the e4m3 ones sit at the 256-register limit: BASELINE configs[4] keeps the static walk).
static inline bool nt_ticket_walk(const NtLaunch& l, NtSchedule s) {
    const int64_t ntm = nt_row_tiles(l), ntn = nt_col_tiles(l), tiles = ntm * ntn;
    const int64_t grid = tiles < 256 ? (tiles + 7) / 8 * 8 : 256;
    const int64_t ppx = (ntm + 3) / 4;
    const int64_t shortest = nt_grouped(s) ? (ntm - 3 * ppx > 0 ? (ntm - 3 * ppx < ppx ? ntm - 3 * ppx : ppx) : 0) * (ntn / 2)
                                           : (tiles >> 8) * 32 + ((tiles & 255) > 224 ? (tiles & 255) - 224 : 0);
    return grid == 256 && shortest > 128 && l.K >= 4 * NT_BK && !(l.switches & VIPANT_SW_STATIC_WALK);
}

// the schedule of a bf16 ping-pong launch
static inline NtSchedule nt_schedule_bf16(const NtLaunch& l) {
    const int sw = l.switches, epi = l.epilogue;
    if (sw & VIPANT_SW_DEEP_ALWAYS) return NT_DEEP;
    const bool groupable = nt_groupable(l);
    // the column-grouped walk is the default of the c_fc launch (853 vs 870-881 us, step -0.27 ms in-box; the QuickGELU' launch of
    // the same shape does not move: profiles/r2_gemm_experiments.md section 9); GROUPED_ALWAYS forces it everywhere, GROUPED_NEVER
    // turns it off
    // round 5: the two K = 768 launches with 12 column tiles (c_fc + QuickGELU, QuickGELU') run the DEEP schedule ON the column-grouped
    // walk: half of the weight matrix per XCD stays in its L2 (the plain DEEP walk re-streams all of it every round:
    // QuickGELU' fetched 1.93 GB for 0.75 GB of operands) and the look-ahead of DEEP is kept; 878.9 -> 870.2 us and 883.4 -> 872.2 us,
    // alternating in one process, bit-identical (tools/grouped_walk_ab.py).  ROUND4_SCHEDULES: the round-4 choice (grouped k-step / DEEP).
    const bool deep_grouped = groupable && !(sw & (VIPANT_SW_ROUND4_SCHEDULES | VIPANT_SW_GROUPED_NEVER | VIPANT_SW_GROUPED_ALWAYS | VIPANT_SW_DEEP_NEVER));
    if ((epi == VIPANT_EPI_QUICKGELU_D8 || epi == VIPANT_EPI_DQUICKGELU_D8) && deep_grouped) return NT_DEEP_GROUPED;
    // ... and plain launches with >= 8 column tiles (no shape of the ViT-B step: qkv has 9; the ViT-L qkv launch has 12)
    if (epi == VIPANT_EPI_BF16 && deep_grouped && nt_col_tiles(l) >= 8) return NT_DEEP_GROUPED;
    if (groupable && !(sw & VIPANT_SW_GROUPED_NEVER) && (epi == VIPANT_EPI_QUICKGELU_D8 || (sw & VIPANT_SW_GROUPED_ALWAYS))) return NT_KSTEP_GROUPED;
    // the DEEP schedule: -2 ... -5 % on the launches with a long K or a wide N (qkv 608-624 -> 589-603 us, QuickGELU' 933-947 -> 916,
    // dh2 627-634 -> 596-604), +3 % on the 768 x 768 ones, which keep the k-step schedule; DEEP_NEVER: off
    if (!(sw & VIPANT_SW_DEEP_NEVER) && (epi == VIPANT_EPI_DQUICKGELU_D8 || (epi == VIPANT_EPI_BF16 && (l.N >= 1024 || l.K >= 1024))))
        return NT_DEEP;
    return NT_KSTEP;
}

// bf16 operands (vipant_gemm_nt).  The caller has checked the shape and the leading dimensions.
static inline NtRefusal nt_select_bf16(const NtLaunch& l, NtInstance* out) {
    const int sw = l.switches, epi = l.epilogue;
    const bool d8 = epi == VIPANT_EPI_QUICKGELU_D8 || epi == VIPANT_EPI_DQUICKGELU_D8;
    *out = NtInstance{NT_PLAIN, epi, NT_KSTEP, 2, NT_EMIT_NONE, false};
    // FEW_ROWS_BIG_TILES sends few-rows launches through the 256 x 256 kernels again (A/B)
    if (l.few_rows && !(sw & VIPANT_SW_FEW_ROWS_BIG_TILES)) {
        out->family = NT_FEW_ROWS;
        if (epi == VIPANT_EPI_BF16 || epi == VIPANT_EPI_F32) return NT_ACCEPT;
        if (epi == VIPANT_EPI_RESIDUAL_F32) return l.aux_null ? NT_RESIDUAL_NEEDS_AUX : NT_ACCEPT;
        if (d8) return l.aux_null || l.aux_misaligned ? NT_D8_NEEDS_ALIGNED_AUX : NT_ACCEPT;
        return NT_FEW_ROWS_EPILOGUE;
    }
    // the output is staged through LDS and leaves as whole rows, 16 bytes per lane
    const bool staged = l.N % 8 == 0 && l.ldc % 8 == 0;
    bool pp = staged && l.K >= 2 * NT_BK && !(sw & VIPANT_SW_TWO_STAGE);
    switch (epi) {
        case VIPANT_EPI_BF16: break;
        case VIPANT_EPI_QUICKGELU: if (l.aux_null) return NT_QUICKGELU_NEEDS_AUX; break;
        case VIPANT_EPI_DQUICKGELU: if (l.aux_null) return NT_DQUICKGELU_NEEDS_AUX; break;
        case VIPANT_EPI_QUICKGELU_D8:
        case VIPANT_EPI_DQUICKGELU_D8:      // ping-pong only
            if (l.aux_null) return NT_D8_NEEDS_AUX;
            if (!(staged && l.K >= 2 * NT_BK) || l.aux_misaligned) return NT_D8_NEEDS_STAGED;
            pp = true;
            break;
        // one tile per workgroup: the only caller of the residual epilogue on the step's path is the last block on its read-out rows
        // (`batch` rows, a handful of tiles), and the persistent form of this epilogue spilled 42 registers (the fp32 residual tile
        // rides beside the accumulators)
        case VIPANT_EPI_RESIDUAL_F32: if (l.aux_null) return NT_RESIDUAL_NEEDS_AUX; pp = false; break;
        case VIPANT_EPI_F32:
        case VIPANT_EPI_SCALE_F32: pp = false; break;
        default: return NT_UNKNOWN_EPILOGUE;
    }
    if (!pp) return NT_ACCEPT;
    out->family = NT_PINGPONG;
    out->schedule = nt_schedule_bf16(l);
    out->ticket = nt_ticket_walk(l, out->schedule);
    return NT_ACCEPT;
}

// e4m3 operands (vipant_gemm_nt_e4m3): always the ping-pong kernel at ES = 1, on the static walk.  The caller has checked the shape
// (K >= 256, N % 8 == 0), that cq goes with a QuickGELU epilogue and that C is NULL only beside cq.
static inline NtRefusal nt_select_e4m3(const NtLaunch& l, NtInstance* out) {
    const int sw = l.switches, epi = l.epilogue;
    *out = NtInstance{NT_PINGPONG, epi, NT_KSTEP, 1, NT_EMIT_NONE, false};
    const bool groupable = nt_groupable(l);
    if (epi == VIPANT_EPI_BF16) {
        // the DEEP schedule: -2..-4 % at K >= 3072, neutral at K <= 1024; E4M3_KSTEP: off
        // wide outputs (>= 8 column tiles, an even number): DEEP on the column-grouped walk -- the ViT-L qkv launch (N = 3072, K = 1024)
        // 1172 -> 1133 us, bit-identical; at N = 1024 (four column tiles) it gains nothing or loses.  E4M3_WIDE_PLAIN_WALK: off.
        if (sw & VIPANT_SW_E4M3_KSTEP) out->schedule = NT_KSTEP;
        else out->schedule = groupable && nt_col_tiles(l) >= 8 && !(sw & VIPANT_SW_E4M3_WIDE_PLAIN_WALK) ? NT_DEEP_GROUPED : NT_DEEP;
        return NT_ACCEPT;
    }
    if (epi != VIPANT_EPI_QUICKGELU_D8 && epi != VIPANT_EPI_DQUICKGELU_D8) return NT_UNKNOWN_EPILOGUE;
    const bool gelu = epi == VIPANT_EPI_QUICKGELU_D8;
    if (!(!l.aux_null || (l.c_null && !l.cq_null)) || l.aux_misaligned) return NT_D8_NEEDS_ALIGNED_AUX;
    if (l.cq_null) return NT_ACCEPT;
    if (gelu && !l.c_null && l.aux_null) return NT_E4M3_C_WITHOUT_AUX;
    if (gelu && l.c_null && l.aux_null) {       // the e4m3 form alone (a tower that keeps neither g nor the codes)
        out->emit = NT_EMIT_ALONE;
        return NT_ACCEPT;
    }
    // QuickGELU without C: the e4m3 form + the codes; QuickGELU' without C: the e4m3 form alone
    out->emit = !l.c_null ? NT_EMIT_ALSO : (gelu ? NT_EMIT_WITH_CODES : NT_EMIT_ALONE);
    // the column-grouped walk (k-step schedule; half of the weight bytes per XCD): 2186 -> 2149 us and 2329 -> 2305 us at the
    // ViT-L shape, bit-identical; DEEP on the grouped walk gains nothing here.  E4M3_EMIT_PLAIN_WALK: the plain walk.
    if (groupable && !(sw & VIPANT_SW_E4M3_EMIT_PLAIN_WALK)) out->schedule = NT_KSTEP_GROUPED;
    return NT_ACCEPT;
}
