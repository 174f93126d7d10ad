// Stand-alone driver of vipant_amd/csrc/nt_select.h for tests/test_nt_select_cpu.py: no HIP, a host compiler builds it alone.
// stdin: one launch per line, "bf16|e4m3 M N K ldc epilogue few_rows C_null aux_null cq_null aux_misaligned switches";
// stdout: the selected kernel instance, or the refusal, per line.
#include <stdio.h>
#include <string.h>

#include "../vipant_amd/csrc/nt_select.h"

int main() {
    static const char* const refusal[] = {"ACCEPT", "UNKNOWN_EPILOGUE", "FEW_ROWS_EPILOGUE", "RESIDUAL_NEEDS_AUX", "QUICKGELU_NEEDS_AUX",
                                          "DQUICKGELU_NEEDS_AUX", "D8_NEEDS_AUX", "D8_NEEDS_ALIGNED_AUX", "D8_NEEDS_STAGED", "E4M3_C_WITHOUT_AUX"};
    char kind[16];
    long long M, N, K, ldc;
    int epi, few, c_null, aux_null, cq_null, aux_mis, sw;
    while (scanf("%15s %lld %lld %lld %lld %d %d %d %d %d %d %d", kind, &M, &N, &K, &ldc, &epi, &few, &c_null, &aux_null, &cq_null, &aux_mis, &sw) == 12) {
        const NtLaunch l{M, N, K, ldc, epi, few != 0, c_null != 0, aux_null != 0, cq_null != 0, aux_mis != 0, sw};
        NtInstance k;
        const NtRefusal why = strcmp(kind, "e4m3") == 0 ? nt_select_e4m3(l, &k) : nt_select_bf16(l, &k);
        if (why != NT_ACCEPT) printf("refuse %s\n", refusal[why]);
        else if (k.family == NT_PINGPONG)
            printf("pingpong epi=%d sched=%d es=%d emit=%d ticket=%d\n", k.epilogue, (int)k.schedule, k.es, (int)k.emit, (int)k.ticket);
        else printf("%s epi=%d\n", k.family == NT_PLAIN ? "plain" : "few_rows", k.epilogue);
    }
    return 0;
}
