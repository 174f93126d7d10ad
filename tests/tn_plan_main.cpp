// Stand-alone driver of vipant_amd/csrc/tn_plan.h for tests/test_tn_plan_cpu.py: no HIP, a host compiler builds it alone.
// stdin: one launch per line, "bf16|e4m3|pair M P Q factor accumulate"; stdout: every field of its TnPlan per line.
#include <stdio.h>
#include <string.h>

#include "../vipant_amd/csrc/tn_plan.h"

int main() {
    char kind[16];
    long long M, P, Q;
    int factor, accumulate;
    while (scanf("%15s %lld %lld %lld %d %d", kind, &M, &P, &Q, &factor, &accumulate) == 6) {
        const bool pair = strcmp(kind, "pair") == 0;
        const TnPlan pl = tn_plan(M, P, Q, strcmp(kind, "e4m3") == 0 ? TN_BK8 : TN_BK, pair ? 2 : 1, factor, accumulate != 0);
        printf("ntp=%lld ntq=%lld tiles=%lld nk=%d splits=%d per=%d direct=%d slab_bytes=%zu colsum_bytes=%zu workspace_bytes=%zu reduce_blocks=%d "
               "cs_parts=%d cs_stride=%d\n", (long long)pl.ntp, (long long)pl.ntq, (long long)pl.tiles, pl.nk, pl.splits, pl.per, (int)pl.direct,
               pl.slab_bytes, pl.colsum_bytes, pl.workspace_bytes, pl.reduce_blocks, pl.cs_parts, pl.cs_stride);
    }
    return 0;
}
