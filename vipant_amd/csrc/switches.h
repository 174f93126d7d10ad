// The A/B switches of VIPANT_GEMM_VARIANT (a bit mask, timing experiments and bit-identity tests only; 0 = what ships).  Every bit
// the sources read has its name here; DESIGN.md section 9 has the table (what each selects, who reads it).  vipant_amd/_ffi.py
// repeats the names of the values that Python code sets.  Host-only header: nothing from HIP.
#pragma once
#include <stdlib.h>

enum : int {
    VIPANT_SW_SKIP_STORES = 1 << 0,            // device, NT kernels: the tile epilogues store nothing (main-loop timing; results are garbage)
    // (bits 1-3 went with the round-2 persistent NT kernel)
    VIPANT_SW_TWO_STAGE = 1 << 4,              // NT: staged bf16-family launches on the round-1 two-stage (plain) kernel; the two-stage TN kernel it also selected is gone
    VIPANT_SW_GROUPED_ALWAYS = 1 << 11,        // NT bf16: every groupable launch on the column-grouped walk (k-step schedule)
    VIPANT_SW_GROUPED_NEVER = 1 << 12,         // NT bf16: no launch on the column-grouped walk
    VIPANT_SW_E4M3_KSTEP = 1 << 15,            // NT e4m3, plain epilogue: the k-step schedule instead of DEEP
    VIPANT_SW_DEEP_ALWAYS = 1 << 17,           // NT bf16: DEEP (plain walk) for every ping-pong launch
    VIPANT_SW_DEEP_NEVER = 1 << 18,            // NT bf16: no launch on the DEEP schedule
    VIPANT_SW_FEW_ROWS_BIG_TILES = 1 << 21,    // NT: VIPANT_EPI_FEW_ROWS launches through the 256 x 256 kernels, as before round 4
    VIPANT_SW_STATIC_WALK = 1 << 22,           // every persistent kernel (NT bf16, attention backward): static stride instead of tickets
    VIPANT_SW_ROUND4_SCHEDULES = 1 << 23,      // NT bf16: no DEEP on the grouped walk (c_fc: grouped k-step, QuickGELU': plain DEEP)
    VIPANT_SW_E4M3_EMIT_PLAIN_WALK = 1 << 25,  // NT e4m3: the QuickGELU launches that emit the e4m3 form on the plain walk
    VIPANT_SW_E4M3_WIDE_PLAIN_WALK = 1 << 26,  // NT e4m3, plain epilogue: wide launches (>= 8 column tiles) on plain DEEP
    VIPANT_SW_E4M3_GROUPED_UNPAIRED = 1 << 27, // device, NT e4m3 grouped walk: a workgroup's tiles of two rounds are not made neighbours
    VIPANT_SW_E4M3_PLAIN_UNPAIRED = 1 << 28,   // device, NT e4m3 plain walk: the same
    VIPANT_SW_SINGLE_DRAWS = 1 << 29,          // device, NT bf16 ticket walk: plain launches with >= 8 column tiles draw single tickets
};

// read per launch: tests and A/B scripts switch the variable inside one process
static inline int vipant_switches() {
    const char* var = getenv("VIPANT_GEMM_VARIANT");
    return var ? atoi(var) : 0;
}
