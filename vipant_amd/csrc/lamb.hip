// LAMB (You et al., ICLR 2020, Alg. 2) with clipping of the GLOBAL gradient norm, over a list of tensors, as one short launch group that
// leaves the stream only through its results: nothing is allocated, nothing is read back, the clip factor and every trust ratio are
// formed on the device and consumed on the device.
//   G   = sqrt(sum over ALL tensors of the call of sum_i g_i^2)          c = max_grad_norm > 0 ? min(1, max_grad_norm / (G + 1e-6)) : 1
//   g'  = c g                 m = m + (1 - beta1)(g' - m)                v = beta2 v + (1 - beta2) g' g'              (adam.hip's forms)
//   u   = (m / bc1) / (sqrt(v / bc2) + eps) + wd_t p                     phi_t = adapt_t and |p| > 0 and |u| > 0 ? |p| / |u| : 1
//   p   = p - lr_t phi_t u
// Work split: adam.hip's -- the concatenated list in chunks of `chunk` elements, one 256-thread workgroup per chunk, which finds its
// tensor by binary search over chunk_start.  The chunk index is also the index of that chunk's partial sums in the workspace.
// Launches and what each moves per element:
//   1  grad_sq   (max_grad_norm > 0 only)  reads g:                        4 B     gsq[chunk] = sum g^2
//   2  fold_g    (max_grad_norm > 0 only)  one workgroup:                  --      G, c from gsq[0 .. nchunks)
//   3  moments                             reads p g m v, writes m v:     24 B     psq[chunk] = sum p^2, usq[chunk] = sum u^2
//   4  fold_phi                            one workgroup per tensor:       --      phi_t from the tensor's psq / usq
//   5  apply                               reads p m v, writes p:         16 B     u recomputed from the updated m, v and the old p
// 40 B per element with the clip off, 44 B with it on, against Adam's 28.  u is never stored: a pass that wrote it and one that read it
// back would move 8 B per element more than recomputing it from what the apply pass reads anyway.  The gradients are read only (g'
// lives in registers).
// Sums: a thread accumulates its 32 squares of a chunk in fp32 (one fma each), the workgroup adds its 256 accumulators in a fixed tree
// (xor butterfly inside a wave, the four waves in the order (0 + 1) + (2 + 3)); the per-chunk fp32 partials are folded in fp64 in
// ascending chunk order on two levels (thread i of the folding workgroup adds the i-th contiguous run of partials in ascending order,
// thread 0 adds the 256 run sums in ascending order).  No float atomics: which element meets which accumulator depends on the list
// alone, every word of the workspace that is read was written by an earlier launch of the same call, so two calls give the same bits
// whatever the workspace held.  A non-finite G runs through as computed (torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False):
// c = NaN for G = NaN, c = 0 for G = inf).
// The per-tensor record (eight floats, 32 bytes, computed by the host in doubles and rounded once):
//   {lr, 1 / bc1, 1 / sqrt(bc2), eps, wd, adapt (0 / 1), 0, 0}       bc1 = 1 - beta1^step, bc2 = 1 - beta2^step
// Workspace (floats): [0] G  [1] c  [2, 4) unused | phi[ntensors] | gsq[nchunks] | psq[nchunks] | usq[nchunks], every section rounded up
// to four floats.  vipant_grad_norm runs launches 1 and 2 alone on the first and third section: the same partials, the same fold, the
// same bits of G as the step that follows it.
#include <stdlib.h>

#include "common.h"

namespace {

constexpr int THREADS = 256;
enum Pass { GRAD_SQ, MOMENTS, APPLY };

struct LambArgs {
    float* const* p; const float* const* g; float* const* m; float* const* v;
    const int64_t* n; const f32x4* rec; const int32_t* chunk_start;
    int ntensors, chunk;
    float w1, b2, w2;               // 1 - beta1, beta2, 1 - beta2
    const float* scal;              // {G, c}: read by the moments pass when the clip is on; nullptr = c is 1
    const float* phi;               // per tensor: read by the apply pass
    float *gsq, *psq, *usq;         // per chunk
};

struct Coef { float clip, step, rbc1, rsq, eps, wd, w1, b2, w2; };

__host__ __device__ constexpr int64_t round4(int64_t x) { return (x + 3) & ~(int64_t)3; }

__device__ __forceinline__ float lamb_u(float p, float m, float v, const Coef& c) {
    return (m * c.rbc1) / (sqrtf(v) * c.rsq + c.eps) + c.wd * p;
}

template <int PASS>
__device__ __forceinline__ void lamb_one(float& p, float g, float& m, float& v, const Coef& c, float& s0, float& s1) {
    if constexpr (PASS == GRAD_SQ) {
        s0 = fmaf(g, g, s0);
    } else if constexpr (PASS == MOMENTS) {
        g = c.clip * g;
        m = m + c.w1 * (g - m);
        v = c.b2 * v + (c.w2 * g) * g;
        const float u = lamb_u(p, m, v, c);
        s0 = fmaf(p, p, s0);
        s1 = fmaf(u, u, s1);
    } else {
        p = p - c.step * lamb_u(p, m, v, c);
    }
}

template <int VEC>
__device__ __forceinline__ void load(const float* q, float* r) {
    if constexpr (VEC == 4) {
        const f32x4 t = *(const f32x4*)q;
        r[0] = t[0]; r[1] = t[1]; r[2] = t[2]; r[3] = t[3];
    } else {
        r[0] = *q;
    }
}
template <int VEC>
__device__ __forceinline__ void store(float* q, const float* r) {
    if constexpr (VEC == 4) {
        f32x4 t;
        t[0] = r[0]; t[1] = r[1]; t[2] = r[2]; t[3] = r[3];
        *(f32x4*)q = t;
    } else {
        *q = r[0];
    }
}

// What a pass reads and writes at offset i: GRAD_SQ reads g; MOMENTS reads p g m v and writes m v; APPLY reads p m v and writes p.
template <int PASS, int VEC>
__device__ __forceinline__ void load_group(const float* p, const float* g, const float* m, const float* v, int i, float* P, float* G,
                                           float* M, float* V) {
    if constexpr (PASS != APPLY) load<VEC>(g + i, G);
    if constexpr (PASS != GRAD_SQ) { load<VEC>(p + i, P); load<VEC>(m + i, M); load<VEC>(v + i, V); }
}
template <int PASS, int VEC>
__device__ __forceinline__ void store_group(float* p, float* m, float* v, int i, const float* P, const float* M, const float* V) {
    if constexpr (PASS == MOMENTS) { store<VEC>(m + i, M); store<VEC>(v + i, V); }
    if constexpr (PASS == APPLY) store<VEC>(p + i, P);
}

// elements [0, count) of one chunk; VEC = 4 needs every pointer the pass touches 16-byte aligned.  U groups of loads are in flight per
// thread before the first is used.  s0 / s1: this thread's fp32 sums, one accumulator each, in the order the thread meets its elements.
template <int PASS, int VEC, int U>
__device__ __forceinline__ void lamb_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, int count, const Coef& c, float& s0, float& s1) {
    constexpr int STEP = THREADS * VEC;
    int i = (int)threadIdx.x * VEC;
    for (; i + (U - 1) * STEP + VEC <= count; i += U * STEP) {
        float P[U][VEC] = {}, G[U][VEC] = {}, M[U][VEC] = {}, V[U][VEC] = {};
#pragma unroll
        for (int u = 0; u < U; ++u) load_group<PASS, VEC>(p, g, m, v, i + u * STEP, P[u], G[u], M[u], V[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) lamb_one<PASS>(P[u][k], G[u][k], M[u][k], V[u][k], c, s0, s1);
            store_group<PASS, VEC>(p, m, v, i + u * STEP, P[u], M[u], V[u]);
        }
    }
    for (; i + VEC <= count; i += STEP) {
        float P[VEC] = {}, G[VEC] = {}, M[VEC] = {}, V[VEC] = {};
        load_group<PASS, VEC>(p, g, m, v, i, P, G, M, V);
#pragma unroll
        for (int k = 0; k < VEC; ++k) lamb_one<PASS>(P[k], G[k], M[k], V[k], c, s0, s1);
        store_group<PASS, VEC>(p, m, v, i, P, M, V);
    }
    if constexpr (VEC > 1) {               // the count % VEC elements at the end of a tensor's last chunk
        const int j = (count & ~(VEC - 1)) + (int)threadIdx.x;
        if (j < count) {
            float P[1] = {}, G[1] = {}, M[1] = {}, V[1] = {};
            load_group<PASS, 1>(p, g, m, v, j, P, G, M, V);
            lamb_one<PASS>(P[0], G[0], M[0], V[0], c, s0, s1);
            store_group<PASS, 1>(p, m, v, j, P, M, V);
        }
    }
}

// the workgroup's sum of one fp32 value per thread, in a fixed tree; every thread returns it.  `slot`: four floats of LDS per use.
__device__ __forceinline__ float block_sum(float x, float* slot) {
    x = wave_sum(x);
    if ((threadIdx.x & (WAVE - 1)) == 0) slot[threadIdx.x / WAVE] = x;
    __syncthreads();
    return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

template <int PASS, bool WIDE>
__global__ __launch_bounds__(THREADS) void lamb_pass_kernel(LambArgs a) {
    __shared__ float red[8];
    const int b = (int)blockIdx.x;
    int lo = 0, hi = a.ntensors;           // the tensor t with chunk_start[t] <= b < chunk_start[t + 1] (tensors without elements have no chunk)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.chunk_start[mid] <= b) lo = mid; else hi = mid;
    }
    const int t = lo;
    const int64_t off = (int64_t)(b - a.chunk_start[t]) * a.chunk, left = a.n[t] - off;
    float s0 = 0.f, s1 = 0.f;
    if (off >= 0 && left > 0) {            // (a table that does not fit the list: touch no tensor, the chunk's sums are 0)
        const int count = left < a.chunk ? (int)left : a.chunk;
        Coef c{1.f, 0.f, 0.f, 0.f, 0.f, 0.f, a.w1, a.b2, a.w2};
        float *p = nullptr, *m = nullptr, *v = nullptr;
        const float* g = nullptr;
        if constexpr (PASS != GRAD_SQ) {       // (vipant_grad_norm has neither a record nor these tables)
            const f32x4 r0 = a.rec[2 * t], r1 = a.rec[2 * t + 1];
            c.rbc1 = r0[1]; c.rsq = r0[2]; c.eps = r0[3]; c.wd = r1[0];
            if (PASS == MOMENTS && a.scal) c.clip = a.scal[1];
            if (PASS == APPLY) c.step = r0[0] * a.phi[t];
            p = a.p[t] + off; m = a.m[t] + off; v = a.v[t] + off;
        }
        if constexpr (PASS != APPLY) g = a.g[t] + off;
        // chunk starts are multiples of 4 elements, so a chunk is 16-byte aligned exactly when its tensor is
        const uintptr_t touched = (PASS != APPLY ? (uintptr_t)g : 0) | (PASS != GRAD_SQ ? ((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) : 0);
        if (WIDE && (touched & 15) == 0)
            lamb_chunk<PASS, 4, 2>(p, g, m, v, count, c, s0, s1);
        else
            lamb_chunk<PASS, 1, 4>(p, g, m, v, count, c, s0, s1);
    }
    if (PASS == GRAD_SQ) {
        s0 = block_sum(s0, red);
        if (threadIdx.x == 0) a.gsq[b] = s0;
    } else if (PASS == MOMENTS) {
        s0 = block_sum(s0, red);
        s1 = block_sum(s1, red + 4);
        if (threadIdx.x == 0) { a.psq[b] = s0; a.usq[b] = s1; }
    }
}

// part[first .. last) in fp64, ascending on two levels: thread i adds the i-th run of ceil(count / 256) partials, thread `owner` adds
// the 256 run sums and returns the total (the other threads return 0).  `runs`: 256 doubles of LDS per use.
__device__ __forceinline__ double fold_ascending(const float* part, int first, int last, double* runs, int owner) {
    const int64_t count = last > first ? last - first : 0, per = (count + THREADS - 1) / THREADS;
    const int64_t lo = first + (int64_t)threadIdx.x * per, hi = lo + per < last ? lo + per : last;
    double s = 0.0;
    for (int64_t i = lo; i < hi; ++i) s += (double)part[i];
    runs[threadIdx.x] = s;
    __syncthreads();
    double total = 0.0;
    if ((int)threadIdx.x == owner)
        for (int i = 0; i < THREADS; ++i) total += runs[i];
    return total;
}

// G and c from the per-chunk sums of g^2; `out` (optional) receives G as well
__global__ __launch_bounds__(THREADS) void lamb_fold_g_kernel(const float* gsq, int nchunks, float max_grad_norm, float* scal, float* out) {
    __shared__ double runs[THREADS];
    const double total = fold_ascending(gsq, 0, nchunks, runs, 0);
    if (threadIdx.x == 0) {
        const float G = (float)sqrt(total);
        const float x = max_grad_norm / (G + 1e-6f);
        scal[0] = G;
        scal[1] = max_grad_norm > 0.f ? (!(x >= 1.f) ? x : 1.f) : 1.f;          // torch.clamp(x, max=1): a NaN stays a NaN
        if (out) out[0] = G;
    }
}

// phi_t from the tensor's chunks of psq / usq: waves 0 and 1 own one total each
__global__ __launch_bounds__(THREADS) void lamb_fold_phi_kernel(const float* psq, const float* usq, const int32_t* chunk_start,
                                                                const f32x4* rec, int nchunks, float* phi) {
    __shared__ double runs[2][THREADS];
    __shared__ double total[2];
    const int t = (int)blockIdx.x;
    int first = chunk_start[t], last = chunk_start[t + 1];
    first = first < 0 ? 0 : first;
    last = last > nchunks ? nchunks : last;             // (a table that does not fit the workspace: read nothing beyond it)
    const double P = fold_ascending(psq, first, last, runs[0], 0);
    const double U = fold_ascending(usq, first, last, runs[1], WAVE);
    if (threadIdx.x == 0) total[0] = P;
    if (threadIdx.x == WAVE) total[1] = U;
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool adapt = rec[2 * t + 1][1] != 0.f;
        phi[t] = adapt && total[0] > 0.0 && total[1] > 0.0 ? (float)(sqrt(total[0]) / sqrt(total[1])) : 1.f;
    }
}

// Access width of chunks whose pointers are 16-byte aligned: the narrow form by default, for adam.hip's reason (its two widths tie
// within the run-to-run spread on the 88 M-parameter list, and these passes move fewer bytes per element through the same loop);
// VIPANT_LAMB_WIDTH=4|16 (read per call) selects a width for A/B timing and for the tests, which run both.
constexpr bool WIDE_DEFAULT = false;
bool wide_accesses() {
    const char* env = getenv("VIPANT_LAMB_WIDTH");
    if (env && *env) return atoi(env) == 16;
    return WIDE_DEFAULT;
}

template <int PASS>
void launch_pass(const LambArgs& a, int64_t nchunks, bool wide, hipStream_t s) {
    const dim3 grid((unsigned)nchunks), block(THREADS);
    if (wide) hipLaunchKernelGGL((lamb_pass_kernel<PASS, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((lamb_pass_kernel<PASS, false>), grid, block, 0, s, a);
}

int32_t check_tables(const char* who, bool null_table, int64_t ntensors, int64_t nchunks, int64_t chunk) {
    VIPANT_REQUIRE(ntensors > 0 && ntensors < 65536, VIPANT_EBADSHAPE, "%s: bad tensor count %ld", who, (long)ntensors);
    VIPANT_REQUIRE(!null_table, VIPANT_EBADSHAPE, "%s: null table", who);
    VIPANT_REQUIRE(nchunks > 0 && nchunks < ((int64_t)1 << 31), VIPANT_EBADSHAPE, "%s: bad chunk count %ld", who, (long)nchunks);
    VIPANT_REQUIRE(chunk >= 1024 && chunk <= (1 << 20) && chunk % 1024 == 0, VIPANT_EBADSHAPE,
                   "%s: chunk must be a multiple of 1024 in [1024, 2^20], got %ld", who, (long)chunk);
    return VIPANT_OK;
}

}  // namespace

extern "C" size_t vipant_grad_norm_workspace_bytes(int64_t nchunks) {
    return nchunks > 0 ? (size_t)(4 + round4(nchunks)) * sizeof(float) : 0;
}

extern "C" size_t vipant_lamb_workspace_bytes(int64_t ntensors, int64_t nchunks) {
    return ntensors > 0 && nchunks > 0 ? (size_t)(4 + round4(ntensors) + 3 * round4(nchunks)) * sizeof(float) : 0;
}

extern "C" int32_t vipant_grad_norm(const float* const* g, const int64_t* n, const int32_t* chunk_start, int64_t ntensors, int64_t nchunks,
                                    int64_t chunk, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int32_t rc = check_tables("grad_norm", !(g && n && chunk_start && out), ntensors, nchunks, chunk)) return rc;
    VIPANT_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= vipant_grad_norm_workspace_bytes(nchunks),
                   VIPANT_ENOWORKSPACE, "grad_norm: workspace of %zu bytes, 16-byte aligned, needed (got %zu)",
                   vipant_grad_norm_workspace_bytes(nchunks), workspace_bytes);
    float* ws = (float*)workspace;
    LambArgs a{};
    a.g = g; a.n = n; a.chunk_start = chunk_start; a.ntensors = (int)ntensors; a.chunk = (int)chunk; a.gsq = ws + 4;
    hipStream_t s = (hipStream_t)stream;
    launch_pass<GRAD_SQ>(a, nchunks, wide_accesses(), s);
    hipLaunchKernelGGL(lamb_fold_g_kernel, dim3(1), dim3(THREADS), 0, s, a.gsq, (int)nchunks, 0.f, ws, out);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" int32_t vipant_lamb_step(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n,
                                    const float* rec, const int32_t* chunk_start, int64_t ntensors, int64_t nchunks, int64_t chunk,
                                    double beta1, double beta2, double max_grad_norm, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    if (const int32_t rc = check_tables("lamb_step", !(p && g && m && v && n && rec && chunk_start), ntensors, nchunks, chunk)) return rc;
    VIPANT_REQUIRE(((uintptr_t)rec & 15) == 0, VIPANT_EBADSHAPE, "lamb_step: rec must be 16-byte aligned");
    VIPANT_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, VIPANT_EBADSHAPE, "lamb_step: betas must lie in [0, 1)");
    VIPANT_REQUIRE(max_grad_norm >= 0.0, VIPANT_EBADSHAPE, "lamb_step: max_grad_norm must be >= 0 (0 = no clipping), got %g", max_grad_norm);
    VIPANT_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= vipant_lamb_workspace_bytes(ntensors, nchunks),
                   VIPANT_ENOWORKSPACE, "lamb_step: workspace of %zu bytes, 16-byte aligned, needed (got %zu)",
                   vipant_lamb_workspace_bytes(ntensors, nchunks), workspace_bytes);
    float* ws = (float*)workspace;
    float* phi = ws + 4;
    float* gsq = phi + round4(ntensors);
    float* psq = gsq + round4(nchunks);
    float* usq = psq + round4(nchunks);
    const bool clip = max_grad_norm > 0.0, wide = wide_accesses();
    const LambArgs a{p, g, m, v, n, (const f32x4*)rec, chunk_start, (int)ntensors, (int)chunk, (float)(1.0 - beta1), (float)beta2,
                     (float)(1.0 - beta2), clip ? ws : nullptr, phi, gsq, psq, usq};
    hipStream_t s = (hipStream_t)stream;
    if (clip) {
        launch_pass<GRAD_SQ>(a, nchunks, wide, s);
        hipLaunchKernelGGL(lamb_fold_g_kernel, dim3(1), dim3(THREADS), 0, s, gsq, (int)nchunks, (float)max_grad_norm, ws, (float*)nullptr);
    }
    launch_pass<MOMENTS>(a, nchunks, wide, s);
    hipLaunchKernelGGL(lamb_fold_phi_kernel, dim3((unsigned)ntensors), dim3(THREADS), 0, s, psq, usq, chunk_start, a.rec, (int)nchunks, phi);
    launch_pass<APPLY>(a, nchunks, wide, s);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}
