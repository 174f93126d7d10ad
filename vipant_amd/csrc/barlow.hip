// Barlow Twins loss head (cvap/module/decoder/loss_head.py:287-328): batch normalisation over the batch dimension
// (nn.BatchNorm1d in training mode, with the optional ReLU of the projector fused) and the cross-correlation loss with its
// gradient.  Every reduction is deterministic and two-level: partial sums per (64-column group, 64-row chunk) in a fixed order
// into the caller's workspace, then a fixed-order sum of the partials (fp64) -- no float atomics, two runs are bit-identical.
#include "common.h"

#define BN_COLS 64  // columns per workgroup: one lane per column (a wave reads 256 contiguous bytes of a row)
#define BN_ROWS 64  // rows per chunk (grid.y)
#define BN_WAVES 4  // waves per workgroup: wave w takes rows w, w + 4, ... of its chunk

static inline int64_t bn_chunks(int64_t M) { return ceil_div(M, BN_ROWS); }

// (x - mean) * rstd [* gamma + beta]: ONE definition for the forward and the ReLU mask the backward recomputes, so the
// mask sees bit for bit the value the forward rectified
__device__ __forceinline__ float bn_affine(float x, float mean, float rstd, const float* gamma, const float* beta, int col) {
    float v = (x - mean) * rstd;
    if (gamma != nullptr) v = __builtin_fmaf(v, gamma[col], beta != nullptr ? beta[col] : 0.f);
    return v;
}

// forward, level 1: per column sum(x - s) and sum((x - s)^2) over one chunk, s = x[0, col] (a per-column shift shared by all
// chunks: the variance comes from shifted values, so a column mean far from zero costs no precision).  part [chunks][2][N].
__global__ __launch_bounds__(256) void bn_fwd_partial(const float* __restrict__ x, int64_t ldx, float* __restrict__ part,
                                                      int M, int N) {
    __shared__ float sh[2][BN_WAVES][BN_COLS];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int col = blockIdx.x * BN_COLS + tx;
    const int r0 = blockIdx.y * BN_ROWS, r1 = min(r0 + BN_ROWS, M);
    float s = 0.f, q = 0.f;
    if (col < N) {
        const float shift = x[col];
        for (int r = r0 + ty; r < r1; r += BN_WAVES) {
            const float d = x[(int64_t)r * ldx + col] - shift;
            s += d;
            q = __builtin_fmaf(d, d, q);
        }
    }
    sh[0][ty][tx] = s;
    sh[1][ty][tx] = q;
    __syncthreads();
    if (ty < 2 && col < N) {
        const float v = (sh[ty][0][tx] + sh[ty][1][tx]) + (sh[ty][2][tx] + sh[ty][3][tx]);
        part[((int64_t)blockIdx.y * 2 + ty) * N + col] = v;
    }
}

// forward, level 2: every workgroup sums the partials of its 64 columns (fp64, chunk order), normalises its chunk and writes
// bf16; the chunk-0 workgroups also write mean / rstd and update the running statistics (unbiased variance, as torch does).
__global__ __launch_bounds__(256) void bn_fwd_apply(const float* __restrict__ x, int64_t ldx, const float* __restrict__ part,
                                                    int nchunks, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                    int relu, bf16_t* __restrict__ y, float* __restrict__ mean_out,
                                                    float* __restrict__ rstd_out, float* __restrict__ run_mean,
                                                    float* __restrict__ run_var, int64_t* __restrict__ nbt, float momentum,
                                                    float eps, int M, int N) {
    __shared__ float st[2][BN_COLS];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int col = blockIdx.x * BN_COLS + tx;
    if (ty == 0 && col < N) {
        double s = 0.0, q = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            s += (double)part[((int64_t)c * 2 + 0) * N + col];
            q += (double)part[((int64_t)c * 2 + 1) * N + col];
        }
        const double ms = s / M;
        double var = q / M - ms * ms;
        var = var > 0.0 ? var : 0.0;
        const float mean = (float)((double)x[col] + ms);
        const float rstd = (float)(1.0 / sqrt(var + (double)eps));
        st[0][tx] = mean;
        st[1][tx] = rstd;
        if (blockIdx.y == 0) {
            mean_out[col] = mean;
            rstd_out[col] = rstd;
            if (run_mean != nullptr) {
                run_mean[col] = (1.f - momentum) * run_mean[col] + momentum * mean;
                run_var[col] = (1.f - momentum) * run_var[col] + momentum * (float)(var * M / (M - 1));
            }
        }
    }
    if (nbt != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) nbt[0] = nbt[0] + 1;
    __syncthreads();
    if (col >= N) return;
    const float mean = st[0][tx], rstd = st[1][tx];
    const int r0 = blockIdx.y * BN_ROWS, r1 = min(r0 + BN_ROWS, M);
    for (int r = r0 + ty; r < r1; r += BN_WAVES) {
        float v = bn_affine(x[(int64_t)r * ldx + col], mean, rstd, gamma, beta, col);
        if (relu) v = fmaxf(v, 0.f);
        y[(int64_t)r * N + col] = f32_to_bf16(v);
    }
}

// backward, level 1: per column and chunk sum(g), sum(g * xhat) over all rows and over the rows of [row0, row0 + nrows),
// g = dy masked by the recomputed ReLU.  part [chunks][4][N].
__global__ __launch_bounds__(256) void bn_bwd_partial(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ x,
                                                      int64_t ldx, const float* __restrict__ mean_in,
                                                      const float* __restrict__ rstd_in, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int relu, int row0, int row1,
                                                      float* __restrict__ part, int M, int N) {
    __shared__ float sh[4][BN_WAVES][BN_COLS];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int col = blockIdx.x * BN_COLS + tx;
    const int r0 = blockIdx.y * BN_ROWS, r1 = min(r0 + BN_ROWS, M);
    float sg = 0.f, sgx = 0.f, rg = 0.f, rgx = 0.f;
    if (col < N) {
        const float mean = mean_in[col], rstd = rstd_in[col];
        for (int r = r0 + ty; r < r1; r += BN_WAVES) {
            const float xv = x[(int64_t)r * ldx + col];
            const float xhat = (xv - mean) * rstd;
            float g = dy[(int64_t)r * lddy + col];
            if (relu && !(bn_affine(xv, mean, rstd, gamma, beta, col) > 0.f)) g = 0.f;
            sg += g;
            sgx = __builtin_fmaf(g, xhat, sgx);
            if (r >= row0 && r < row1) {
                rg += g;
                rgx = __builtin_fmaf(g, xhat, rgx);
            }
        }
    }
    sh[0][ty][tx] = sg;
    sh[1][ty][tx] = sgx;
    sh[2][ty][tx] = rg;
    sh[3][ty][tx] = rgx;
    __syncthreads();
    if (col < N) {
        const float v = (sh[ty][0][tx] + sh[ty][1][tx]) + (sh[ty][2][tx] + sh[ty][3][tx]);
        part[((int64_t)blockIdx.y * 4 + ty) * N + col] = v;
    }
}

// backward, level 2: dx = rstd * gamma * (g - sum(g) / M - xhat * sum(g xhat) / M) over the chunk (column sums over ALL rows);
// the chunk-0 workgroups write d gamma = sum(g xhat), d beta = sum(g) over the row range.
__global__ __launch_bounds__(256) void bn_bwd_apply(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ x,
                                                    int64_t ldx, const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                    const float* __restrict__ part, int nchunks, bf16_t* __restrict__ dx,
                                                    float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate,
                                                    int M, int N) {
    __shared__ float st[2][BN_COLS];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int col = blockIdx.x * BN_COLS + tx;
    if (ty == 0 && col < N) {
        double sg = 0.0, sgx = 0.0, rg = 0.0, rgx = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            const float* p = part + (int64_t)c * 4 * N + col;
            sg += (double)p[0];
            sgx += (double)p[N];
            rg += (double)p[2 * N];
            rgx += (double)p[3 * N];
        }
        st[0][tx] = (float)(sg / M);
        st[1][tx] = (float)(sgx / M);
        if (blockIdx.y == 0 && dgamma != nullptr) {
            dgamma[col] = (accumulate ? dgamma[col] : 0.f) + (float)rgx;
            dbeta[col] = (accumulate ? dbeta[col] : 0.f) + (float)rg;
        }
    }
    __syncthreads();
    if (col >= N) return;
    const float mean = mean_in[col], rstd = rstd_in[col];
    const float mg = st[0][tx], mgx = st[1][tx];
    const float scale = rstd * (gamma != nullptr ? gamma[col] : 1.f);
    const int r0 = blockIdx.y * BN_ROWS, r1 = min(r0 + BN_ROWS, M);
    for (int r = r0 + ty; r < r1; r += BN_WAVES) {
        const float xv = x[(int64_t)r * ldx + col];
        const float xhat = (xv - mean) * rstd;
        float g = dy[(int64_t)r * lddy + col];
        if (relu && !(bn_affine(xv, mean, rstd, gamma, beta, col) > 0.f)) g = 0.f;
        dx[(int64_t)r * N + col] = f32_to_bf16(scale * (g - mg - xhat * mgx));
    }
}

// ---- cross-correlation loss -------------------------------------------------------------------------------------------
// One 64 x 64 tile of c per workgroup: v = c / M; on-diagonal (v - 1)^2, off-diagonal v^2, partial sums per tile into
// part[tile][2]; with G != NULL also g = d loss / d v * (1 / M) * grad_scale, written as G (row-major) and, through LDS, as G^T.
__global__ __launch_bounds__(256) void barlow_tile(const float* __restrict__ c, int64_t ldc, int N, float inv_m, float lambd,
                                                   const float* __restrict__ grad_scale, float* __restrict__ part,
                                                   bf16_t* __restrict__ G, bf16_t* __restrict__ Gt) {
    __shared__ float tile[64][65];
    __shared__ float red[2][256];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    const int j = j0 + tx;
    const float gs = (grad_scale != nullptr ? grad_scale[0] : 1.f) * inv_m;
    float on = 0.f, off = 0.f;
#pragma unroll 4
    for (int k = 0; k < 64; k += BN_WAVES) {
        const int i = i0 + ty + k;
        float g = 0.f;
        if (i < N && j < N) {
            const float v = c[(int64_t)i * ldc + j] * inv_m;
            if (i == j) {
                const float d = v - 1.f;
                on = __builtin_fmaf(d, d, on);
                g = 2.f * d;
            } else {
                off = __builtin_fmaf(v, v, off);
                g = 2.f * lambd * v;
            }
            g *= gs;
            if (G != nullptr) G[(int64_t)i * N + j] = f32_to_bf16(g);
        }
        tile[ty + k][tx] = g;
    }
    red[0][threadIdx.x] = on;
    red[1][threadIdx.x] = off;
    __syncthreads();
    if (Gt != nullptr) {
        const int ii = i0 + tx;
#pragma unroll 4
        for (int k = 0; k < 64; k += BN_WAVES) {
            const int jj = j0 + ty + k;
            if (ii < N && jj < N) Gt[(int64_t)jj * N + ii] = f32_to_bf16(tile[tx][ty + k]);
        }
    }
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int64_t t = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[2 * t] = red[0][0];
        part[2 * t + 1] = red[1][0];
    }
}

// level 2: one workgroup sums the tile partials in a fixed order (fp64): loss[0] = on + lambd * off, loss[1] = on, loss[2] = off
__global__ __launch_bounds__(256) void barlow_finish(const float* __restrict__ part, int64_t ntiles, float lambd,
                                                     float* __restrict__ loss) {
    __shared__ double red[2][256];
    double on = 0.0, off = 0.0;
    for (int64_t t = threadIdx.x; t < ntiles; t += 256) {
        on += (double)part[2 * t];
        off += (double)part[2 * t + 1];
    }
    red[0][threadIdx.x] = on;
    red[1][threadIdx.x] = off;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        loss[0] = (float)(red[0][0] + (double)lambd * red[1][0]);
        loss[1] = (float)red[0][0];
        loss[2] = (float)red[1][0];
    }
}

// ---- host entry points ------------------------------------------------------------------------------------------------
extern "C" size_t vipant_batchnorm_workspace_bytes(int64_t M, int64_t N) {
    return (size_t)(bn_chunks(M > 0 ? M : 1) * 4 * (N > 0 ? N : 1) * sizeof(float));
}

static int32_t bn_check(const char* who, int64_t M, int64_t N, int64_t ldx, size_t need, void* workspace, size_t workspace_bytes) {
    VIPANT_REQUIRE(M >= 2 && N > 0, VIPANT_EBADSHAPE, "%s: training-mode batch norm needs M >= 2 rows and N > 0 (M=%ld N=%ld)",
                   who, (long)M, (long)N);
    VIPANT_REQUIRE(M < (1ll << 31) && N < (1ll << 31) && ldx >= N, VIPANT_EBADSHAPE, "%s: bad shape M=%ld N=%ld ldx=%ld", who,
                   (long)M, (long)N, (long)ldx);
    VIPANT_REQUIRE(ceil_div(N, BN_COLS) < 65536 * 1024ll && bn_chunks(M) < 65536, VIPANT_EBADSHAPE, "%s: grid too large", who);
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= need, VIPANT_ENOWORKSPACE,
                   "%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
    return VIPANT_OK;
}

extern "C" int32_t vipant_batchnorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, int32_t relu,
                                        uint16_t* y, float* mean, float* rstd, float* running_mean, float* running_var,
                                        int64_t* num_batches_tracked, float momentum, float eps, int64_t M, int64_t N,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    int32_t rc = bn_check("batchnorm_fwd", M, N, ldx, vipant_batchnorm_workspace_bytes(M, N), workspace, workspace_bytes);
    if (rc != VIPANT_OK) return rc;
    VIPANT_REQUIRE(x != nullptr && y != nullptr && mean != nullptr && rstd != nullptr, VIPANT_EBADSHAPE,
                   "batchnorm_fwd: x, y, mean and rstd are required");
    VIPANT_REQUIRE((gamma == nullptr) == (beta == nullptr), VIPANT_EBADSHAPE, "batchnorm_fwd: gamma and beta go together");
    VIPANT_REQUIRE((running_mean == nullptr) == (running_var == nullptr), VIPANT_EBADSHAPE,
                   "batchnorm_fwd: running_mean and running_var go together");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(N, BN_COLS), (unsigned)bn_chunks(M));
    float* part = (float*)workspace;
    hipLaunchKernelGGL(bn_fwd_partial, grid, dim3(256), 0, s, x, ldx, part, (int)M, (int)N);
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_fwd_apply, grid, dim3(256), 0, s, x, ldx, part, (int)grid.y, gamma, beta, (int)(relu != 0), (bf16_t*)y,
                       mean, rstd, running_mean, running_var, num_batches_tracked, momentum, eps, (int)M, (int)N);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" int32_t vipant_batchnorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* mean,
                                        const float* rstd, const float* gamma, const float* beta, int32_t relu, uint16_t* dx,
                                        float* dgamma, float* dbeta, int64_t row0, int64_t nrows, int32_t accumulate, int64_t M,
                                        int64_t N, void* workspace, size_t workspace_bytes, void* stream) {
    int32_t rc = bn_check("batchnorm_bwd", M, N, ldx, vipant_batchnorm_workspace_bytes(M, N), workspace, workspace_bytes);
    if (rc != VIPANT_OK) return rc;
    VIPANT_REQUIRE(dy != nullptr && x != nullptr && mean != nullptr && rstd != nullptr && dx != nullptr && lddy >= N,
                   VIPANT_EBADSHAPE, "batchnorm_bwd: dy, x, mean, rstd and dx are required (lddy >= N)");
    VIPANT_REQUIRE((gamma == nullptr) == (beta == nullptr), VIPANT_EBADSHAPE, "batchnorm_bwd: gamma and beta go together");
    VIPANT_REQUIRE((dgamma == nullptr) == (dbeta == nullptr) && (dgamma == nullptr || gamma != nullptr), VIPANT_EBADSHAPE,
                   "batchnorm_bwd: dgamma and dbeta go together and need gamma");
    VIPANT_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= M, VIPANT_EBADSHAPE,
                   "batchnorm_bwd: row range [%ld, %ld) outside [0, %ld)", (long)row0, (long)(row0 + nrows), (long)M);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div(N, BN_COLS), (unsigned)bn_chunks(M));
    float* part = (float*)workspace;
    hipLaunchKernelGGL(bn_bwd_partial, grid, dim3(256), 0, s, dy, lddy, x, ldx, mean, rstd, gamma, beta, (int)(relu != 0),
                       (int)row0, (int)(row0 + nrows), part, (int)M, (int)N);
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_apply, grid, dim3(256), 0, s, dy, lddy, x, ldx, mean, rstd, gamma, beta, (int)(relu != 0), part,
                       (int)grid.y, (bf16_t*)dx, dgamma, dbeta, (int)(accumulate != 0), (int)M, (int)N);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}

extern "C" size_t vipant_barlow_loss_workspace_bytes(int64_t N) {
    const int64_t t = ceil_div(N > 0 ? N : 1, 64);
    return (size_t)(t * t * 2 * sizeof(float));
}

extern "C" int32_t vipant_barlow_loss(const float* c, int64_t ldc, int64_t M, float lambd, float* loss, const float* grad_scale,
                                      uint16_t* G, uint16_t* Gt, int64_t N, void* workspace, size_t workspace_bytes, void* stream) {
    VIPANT_REQUIRE(M > 0 && N > 0 && N < 65536 * 64ll && ldc >= N, VIPANT_EBADSHAPE, "barlow_loss: bad shape M=%ld N=%ld ldc=%ld",
                   (long)M, (long)N, (long)ldc);
    VIPANT_REQUIRE(c != nullptr && loss != nullptr, VIPANT_EBADSHAPE, "barlow_loss: c and loss are required");
    VIPANT_REQUIRE((G == nullptr) == (Gt == nullptr), VIPANT_EBADSHAPE, "barlow_loss: G and Gt go together");
    const size_t need = vipant_barlow_loss_workspace_bytes(N);
    VIPANT_REQUIRE(workspace != nullptr && workspace_bytes >= need, VIPANT_ENOWORKSPACE,
                   "barlow_loss: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
    const unsigned t = (unsigned)ceil_div(N, 64);
    float* part = (float*)workspace;
    hipLaunchKernelGGL(barlow_tile, dim3(t, t), dim3(256), 0, s, c, ldc, (int)N, (float)(1.0 / (double)M), lambd, grad_scale, part,
                       (bf16_t*)G, (bf16_t*)Gt);
    VIPANT_LAUNCH_CHECK();
    hipLaunchKernelGGL(barlow_finish, dim3(1), dim3(256), 0, s, part, (int64_t)t * t, lambd, loss);
    VIPANT_LAUNCH_CHECK();
    return VIPANT_OK;
}
