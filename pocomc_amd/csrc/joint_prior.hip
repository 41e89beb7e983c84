// A flow prior on some columns of x and scipy factors on the others (pocomc_amd/prior.py: JointPrior):
//   log p(x) = [flow.log_prob(u(x_F)) - log|dx_F/du|] + sum_m dist_m.logpdf(x_R[m]),   u = Reparameterize.forward(x_F),
// F the flow block's columns, R the rest.  Two launches around the flow's own forward kernel, as in flow_prior.hip:
// joint_prior_pre_kernel reads the tile of x once and does both parts' elements and row sums, joint_prior_post_kernel joins
// them with the flow's float32 log-density.
#include "pmc_internal.h"
#include "flow_prior_body.h"
#include "prior_body.h"

static inline size_t joint_prior_lds_bytes(int Df, int Dr) {
    const int D = Df + Dr;
    return (size_t)FP_ROWS * (D | 1) * sizeof(double) + (size_t)FP_ROWS * Df * sizeof(float) + FP_ROWS * sizeof(int) +
           (size_t)D * sizeof(int);
}

// The elements of one thread that holds a rest factor: factor m of the rows r0, r0 + rpp, ..., read from tile column jt.
// The factor's term replaces x in T; a row with an x that is not finite or a term that is NaN is marked in rowin (a term
// of -inf is the factor's own support: it stays in the sum).  A loop of its own, for the reason flow_prior_feature gives.
__device__ __forceinline__ void joint_prior_rest_elements(const pmc_prior_t& rest, double* T, int* rowin, int r0, int rpp,
                                                          int rows, int jt, int m, int LD) {
#pragma unroll 1
    for (int r = r0; r < rows; r += rpp) {
        const double xv = T[r * LD + jt];
        const double term = prior_term_any(rest, m, xv);
        T[r * LD + jt] = term;
        if (!isfinite(xv) || isnan(term)) rowin[r] = 0;
    }
}

// flow_prior_pre_kernel's shape (flow_prior.hip): 64 rows of all D = Df + Dr columns through LDS, read with the same two
// coalesced walks, the tile's row length odd (D | 1 doubles) for the rows-first stores and the one-lane-per-row sums.  A
// thread keeps ONE slot c of the rows tid / D, + rpp, ...: slot c < Df is flow feature c in tile column flow_cols[c], slot
// Df + m is rest factor m in tile column rest_cols[m].  The slot's column is fetched with the feature's constants, ahead of
// the barrier, and kept in LDS (cmap) for the row sums.  Within a row the slots' columns are distinct, so an element's
// result replaces its own x and nothing else.  A row's sums are added by one lane in slot order -- the flow terms k = 0,
// ..., Df - 1 as flow_prior_pre_kernel adds them, the rest terms m = 0, ..., Dr - 1 from 0.0 as prior_logpdf_kernel does:
// the row's bits do not depend on the layout, on n or on the row's place in the block.
// A column outside [0, D) (the maps are the caller's: pocomc_amd.JointPrior.layout checks them) is not followed: its slot
// marks every row of the block outside.
// Every barrier is reached by every thread: no branch around one depends on the data.
__global__ __launch_bounds__(FP_THREADS) void joint_prior_pre_kernel(
    pmc_scaler_t s, const int32_t* __restrict__ flow_cols, pmc_prior_t rest, const int32_t* __restrict__ rest_cols,
    const double* __restrict__ x, int64_t row_stride, int64_t col_stride, int64_t n, float* __restrict__ u32,
    double* __restrict__ ldj, double* __restrict__ rest_logp, int32_t* __restrict__ inside) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int Df = s.D, Dr = rest.D, D = Df + Dr, LD = D | 1;
    double* T = sm;                                                       // [FP_ROWS][LD]: x, then J / the factor's term
    float* U = reinterpret_cast<float*>(sm + (size_t)FP_ROWS * LD);       // [FP_ROWS][Df]
    int* rowin = reinterpret_cast<int*>(U + (size_t)FP_ROWS * Df);        // [FP_ROWS]
    int* cmap = rowin + FP_ROWS;                                          // [D]: tile column of every slot
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * FP_ROWS;
    const int rows = (int)min((int64_t)FP_ROWS, n - row0);
    if (tid < FP_ROWS) rowin[tid] = 1;
    const int rpp = FP_THREADS / D;                                       // (D <= 157 < FP_THREADS)
    const int r0 = tid / D, c = tid - r0 * D;
    const bool act = r0 < rpp, is_flow = c < Df;
    ScalerFeat f;
    int col = 0;
    if (act) {
        col = is_flow ? flow_cols[c] : rest_cols[c - Df];
        if (is_flow) scaler_feat_request(f, s, (const pmc_prior_un_t*)nullptr, c);
    }
    const bool col_ok = (unsigned)col < (unsigned)D;
    if (tid < D) cmap[tid] = col_ok ? col : 0;                            // (tid < D: r0 == 0, c == tid)
    if (col_stride == 1) {
        int r = tid / D, cc = tid - r * D;                                // element e = r * D + cc, stepped without a division
        const int dr = FP_THREADS / D, dc = FP_THREADS - dr * D;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            T[r * LD + cc] = x[(row0 + r) * row_stride + cc];
            r += dr; cc += dc;
            if (cc >= D) { cc -= D; ++r; }
        }
    } else {
        int cc = tid / rows, r = tid - cc * rows;                         // element e = cc * rows + r
        const int dc = FP_THREADS / rows, dr = FP_THREADS - dc * rows;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            T[r * LD + cc] = x[(row0 + r) * row_stride + (int64_t)cc * col_stride];
            cc += dc; r += dr;
            if (r >= rows) { r -= rows; ++cc; }
        }
    }
    __syncthreads();
    if (act) {
        if (!col_ok) {
            for (int r = r0; r < rows; r += rpp) rowin[r] = 0;
        } else if (is_flow) {
            scaler_feat_finish(f, s, false);
            flow_prior_feature(f, s, T, U, rowin, r0, rpp, rows, col, c, Df, LD);
        } else {
            joint_prior_rest_elements(rest, T, rowin, r0, rpp, rows, col, c - Df, LD);
        }
    }
    __syncthreads();
    if (tid < rows) {
        const double* a = T + (size_t)tid * LD;
        double l = 0.0;
        for (int k = 0; k < Df; ++k) l += a[cmap[k]];
        if (s.scale) l = s.sum_log_sigma + l;
        double lp = 0.0;
        for (int m = 0; m < Dr; ++m) lp += a[cmap[Df + m]];
        const int in = rowin[tid];
        ldj[row0 + tid] = l;
        rest_logp[row0 + tid] = in ? lp : -INFINITY;
        inside[row0 + tid] = in;
    }
    // the block's rows are one contiguous piece of u32; a row outside the support goes out as zeros
    float* out = u32 + row0 * Df;
    {
        int r = tid / Df, cc = tid - r * Df;
        const int dr = FP_THREADS / Df, dc = FP_THREADS - dr * Df;
        for (int e = tid; e < rows * Df; e += FP_THREADS) {
            out[e] = rowin[r] ? U[e] : 0.0f;
            r += dr; cc += dc;
            if (cc >= Df) { cc -= Df; ++r; }
        }
    }
}

__global__ __launch_bounds__(256) void joint_prior_post_kernel(const float* __restrict__ lp32, const double* __restrict__ ldj,
                                                               const double* __restrict__ rest_logp,
                                                               const int32_t* __restrict__ inside, double* __restrict__ logp,
                                                               int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    logp[r] = joint_prior_join(lp32[r], ldj[r], rest_logp[r], inside[r]);
}

extern "C" int pmc_joint_prior_pre(const pmc_scaler_t* s, const int32_t* flow_cols, const pmc_prior_t* rest,
                                   const int32_t* rest_cols, const double* x, int64_t row_stride, int64_t col_stride,
                                   int64_t n, float* u32, double* ldj, double* rest_logp, int32_t* inside, void* stream) {
    if (!s || !s->low || !s->high || !s->kind || !s->log_width || !flow_cols)
        return pmc_fail("pmc_joint_prior_pre: bad scaler descriptor");
    if (!rest || !rest->family || !rest->loc || !rest->scale || !rest_cols || rest->n_extended < 0)
        return pmc_fail("pmc_joint_prior_pre: bad prior descriptor");
    if (s->D < 2) return pmc_fail("pmc_joint_prior_pre: the flow block needs at least 2 columns (Df >= 2)");
    if (rest->D < 1) return pmc_fail("pmc_joint_prior_pre: the rest needs at least 1 factor (Dr >= 1)");
    if ((int64_t)s->D + rest->D > FP_MAX_D) return pmc_fail("pmc_joint_prior_pre: n_dim too large (Df + Dr <= 157)");
    if (rest->n_extended > 0 && !rest->par)
        return pmc_fail("pmc_joint_prior_pre: factors other than uniform / normal need the parameter table (par)");
    if (s->scale && (!s->mu || !s->sigma)) return pmc_fail("pmc_joint_prior_pre: scale=1 needs mu and sigma");
    if (n == 0) return 0;
    if (!x || !u32 || !ldj || !rest_logp || !inside || n < 0 || row_stride < 0 || col_stride < 0)
        return pmc_fail("pmc_joint_prior_pre: bad argument");
    if ((n + FP_ROWS - 1) / FP_ROWS > 0x7fffffffLL) return pmc_fail("pmc_joint_prior_pre: too many rows for one launch");
    const size_t lds = joint_prior_lds_bytes(s->D, rest->D);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(joint_prior_pre_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return pmc_fail_hip(e, "hipFuncSetAttribute(joint_prior_pre_kernel)");
    }
    hipLaunchKernelGGL(joint_prior_pre_kernel, dim3((unsigned)((n + FP_ROWS - 1) / FP_ROWS)), dim3(FP_THREADS), lds,
                       (hipStream_t)stream, *s, flow_cols, *rest, rest_cols, x, row_stride, col_stride, n, u32, ldj, rest_logp,
                       inside);
    return pmc_check_launch("joint_prior_pre_kernel");
}

extern "C" int pmc_joint_prior_post(const float* lp32, const double* ldj, const double* rest_logp, const int32_t* inside,
                                    double* logp, int64_t n, void* stream) {
    if (n == 0) return 0;
    if (!lp32 || !ldj || !rest_logp || !inside || !logp || n < 0) return pmc_fail("pmc_joint_prior_post: bad argument");
    if ((n + 255) / 256 > 0x7fffffffLL) return pmc_fail("pmc_joint_prior_post: too many rows for one launch");
    hipLaunchKernelGGL(joint_prior_post_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       lp32, ldj, rest_logp, inside, logp, n);
    return pmc_check_launch("joint_prior_post_kernel");
}

// ---------------------------------------------------------------------------------------------------------------
// Several flow blocks and an optional table in one prior (pocomc_amd.JointPrior, the blocks form):
//   log p(x) = sum_b [flow_b.log_prob(u_b(x_{F_b})) - log|dx_{F_b}/du_b|] + sum_m dist_m.logpdf(x_R[m]).
// B + 2 launches: joint_blocks_pre_kernel, every block's own forward kernel, joint_blocks_post_kernel.

// What the pre kernel takes of the host's pmc_joint_blocks_t: the blocks' scalers by value, their column maps, the first
// slot of every block (off[b], off[n_blocks] = the number of flow slots) and the table.
struct JointBlocksArgs {
    pmc_scaler_t s[PMC_JOINT_BLOCKS_MAX];
    const int32_t* cols[PMC_JOINT_BLOCKS_MAX];
    int32_t off[PMC_JOINT_BLOCKS_MAX + 1];
    int32_t n_blocks;
    int32_t D;                                     // the columns of x (>= the slots: the blocks' features and the factors)
    pmc_prior_t rest;
    const int32_t* rest_cols;
};

// joint_prior_lds_bytes with the tile as wide as x: the same bytes where the slots cover every column
static inline size_t joint_blocks_lds_bytes(int DF, int Dr, int D) {
    return (size_t)FP_ROWS * (D | 1) * sizeof(double) + (size_t)FP_ROWS * DF * sizeof(float) + FP_ROWS * sizeof(int) +
           (size_t)(DF + Dr) * sizeof(int);
}

// joint_prior_pre_kernel's shape and stride contract with the flow slots of several blocks: slot c in [off[b], off[b + 1])
// is feature c - off[b] of block b in tile column cols[b][c - off[b]], the slots behind off[B] are the rest factors.  A
// thread finds its block in a loop over the blocks that every lane of the wavefront walks alike (the kernel arguments are
// read with a constant index; a lane keeps the pointers and flags of the block its slot lies in), then does what
// joint_prior_pre_kernel's thread does with that block's constants -- its own transform, its own affine part.  U holds
// block b's [FP_ROWS][Df_b] piece at FP_ROWS * off[b]: the piece leaves as one contiguous run of the block's array, which
// starts n * off[b] floats into u32.  x may have columns that are nobody's slot (a.D > S, the slots' number: columns of a
// Gaussian block, gauss_prior.hip): they go through the tile and are not read.  One lane per row forms block after block's log-determinant, k in slot order as
// flow_prior_pre_kernel adds them, and then the rest's sum: no atomics, a row's bits depend on its values alone.
__global__ __launch_bounds__(FP_THREADS) void joint_blocks_pre_kernel(
    JointBlocksArgs a, const double* __restrict__ x, int64_t row_stride, int64_t col_stride, int64_t n,
    float* __restrict__ u32, double* __restrict__ ldj, double* __restrict__ rest_logp, int32_t* __restrict__ inside) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int B = a.n_blocks, DF = a.off[B], Dr = a.rest.D, S = DF + Dr, D = a.D, LD = D | 1;
    double* T = sm;                                                       // [FP_ROWS][LD]: x, then J / the factor's term
    float* U = reinterpret_cast<float*>(sm + (size_t)FP_ROWS * LD);       // [FP_ROWS * DF]: block after block
    int* rowin = reinterpret_cast<int*>(U + (size_t)FP_ROWS * DF);        // [FP_ROWS]
    int* cmap = rowin + FP_ROWS;                                          // [S]: tile column of every slot
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * FP_ROWS;
    const int rows = (int)min((int64_t)FP_ROWS, n - row0);
    if (tid < FP_ROWS) rowin[tid] = 1;
    const int rpp = FP_THREADS / S;                                       // (S <= D <= 157 < FP_THREADS)
    const int r0 = tid / S, c = tid - r0 * S;
    const bool act = r0 < rpp, is_flow = c < DF;
    // the slot's block: its scaler as this lane's own descriptor, its map, its first slot
    pmc_scaler_t s = a.s[0];
    const int32_t* cols = a.cols[0];
    int o = 0;
#pragma unroll
    for (int b = 1; b < PMC_JOINT_BLOCKS_MAX; ++b) {
        if (b < B && c >= a.off[b]) {
            s = a.s[b];
            cols = a.cols[b];
            o = a.off[b];
        }
    }
    const int cb = c - o, Db = s.D;                                       // (a rest slot keeps the last block's: never used)
    ScalerFeat f;
    int col = 0;
    if (act) {
        col = is_flow ? cols[cb] : a.rest_cols[c - DF];
        if (is_flow) scaler_feat_request(f, s, (const pmc_prior_un_t*)nullptr, cb);
    }
    const bool col_ok = (unsigned)col < (unsigned)D;
    if (tid < S) cmap[tid] = col_ok ? col : 0;                            // (tid < S: r0 == 0, c == tid)
    if (col_stride == 1) {
        int r = tid / D, cc = tid - r * D;                                // element e = r * D + cc, stepped without a division
        const int dr = FP_THREADS / D, dc = FP_THREADS - dr * D;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            T[r * LD + cc] = x[(row0 + r) * row_stride + cc];
            r += dr; cc += dc;
            if (cc >= D) { cc -= D; ++r; }
        }
    } else {
        int cc = tid / rows, r = tid - cc * rows;                         // element e = cc * rows + r
        const int dc = FP_THREADS / rows, dr = FP_THREADS - dc * rows;
        for (int e = tid; e < rows * D; e += FP_THREADS) {
            T[r * LD + cc] = x[(row0 + r) * row_stride + (int64_t)cc * col_stride];
            cc += dc; r += dr;
            if (r >= rows) { r -= rows; ++cc; }
        }
    }
    __syncthreads();
    if (act) {
        if (!col_ok) {
            for (int r = r0; r < rows; r += rpp) rowin[r] = 0;
        } else if (is_flow) {
            scaler_feat_finish(f, s, false);
            flow_prior_feature(f, s, T, U + (size_t)FP_ROWS * o, rowin, r0, rpp, rows, col, cb, Db, LD);
        } else {
            joint_prior_rest_elements(a.rest, T, rowin, r0, rpp, rows, col, c - DF, LD);
        }
    }
    __syncthreads();
    if (tid < rows) {
        const double* t = T + (size_t)tid * LD;
#pragma unroll
        for (int b = 0; b < PMC_JOINT_BLOCKS_MAX; ++b) {
            if (b < B) {
                double l = 0.0;
                for (int k = a.off[b]; k < a.off[b + 1]; ++k) l += t[cmap[k]];
                if (a.s[b].scale) l = a.s[b].sum_log_sigma + l;
                ldj[(int64_t)b * n + row0 + tid] = l;
            }
        }
        const int in = rowin[tid];
        if (Dr > 0) {
            double lp = 0.0;
            for (int m = 0; m < Dr; ++m) lp += t[cmap[DF + m]];
            rest_logp[row0 + tid] = in ? lp : -INFINITY;
        }
        inside[row0 + tid] = in;
    }
    // the block's rows are one contiguous piece of every flow block's array; a row outside the support goes out as zeros
#pragma unroll
    for (int b = 0; b < PMC_JOINT_BLOCKS_MAX; ++b) {
        if (b < B) {
            const int ob = a.off[b], Df = a.off[b + 1] - ob;
            float* out = u32 + n * ob + row0 * Df;
            const float* Ub = U + (size_t)FP_ROWS * ob;
            int r = tid / Df, cc = tid - r * Df;
            const int dr = FP_THREADS / Df, dc = FP_THREADS - dr * Df;
            for (int e = tid; e < rows * Df; e += FP_THREADS) {
                out[e] = rowin[r] ? Ub[e] : 0.0f;
                r += dr; cc += dc;
                if (cc >= Df) { cc -= Df; ++r; }
            }
        }
    }
}

__global__ __launch_bounds__(256) void joint_blocks_post_kernel(int n_blocks, const float* __restrict__ lp32,
                                                                const double* __restrict__ ldj,
                                                                const double* __restrict__ rest_logp,
                                                                const int32_t* __restrict__ inside, double* __restrict__ logp,
                                                                int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    logp[r] = joint_blocks_join(n_blocks, lp32, ldj, rest_logp, inside[r], n, r);
}

// The descriptor's own refusals, shared with the step's stage check (step.hip): 0, or pmc_fail's code with the text set.
int pmc_joint_blocks_check(const pmc_joint_blocks_t* j, int* DF_out, int* Dr_out) {
    if (!j) return pmc_fail("pmc_joint_blocks_pre: bad descriptor");
    if (j->n_blocks < 1 || j->n_blocks > PMC_JOINT_BLOCKS_MAX)
        return pmc_fail("pmc_joint_blocks_pre: n_blocks must lie in 1 .. 8");
    int64_t DF = 0;
    for (int b = 0; b < j->n_blocks; ++b) {
        const pmc_scaler_t* s = j->scaler[b];
        if (!s || !s->low || !s->high || !s->kind || !s->log_width || !j->cols[b])
            return pmc_fail("pmc_joint_blocks_pre: bad scaler descriptor");
        if (s->D < 2) return pmc_fail("pmc_joint_blocks_pre: every flow block needs at least 2 columns (Df >= 2)");
        if (s->scale && (!s->mu || !s->sigma)) return pmc_fail("pmc_joint_blocks_pre: scale=1 needs mu and sigma");
        DF += s->D;
    }
    const pmc_prior_t* rest = j->rest;
    if ((rest == nullptr) != (j->rest_cols == nullptr))
        return pmc_fail("pmc_joint_blocks_pre: rest and rest_cols go together (both, or both NULL)");
    if (rest && (!rest->family || !rest->loc || !rest->scale || rest->n_extended < 0 || rest->D < 1))
        return pmc_fail("pmc_joint_blocks_pre: bad prior descriptor");
    const int64_t Dr = rest ? rest->D : 0;
    if (DF + Dr > FP_MAX_D) return pmc_fail("pmc_joint_blocks_pre: n_dim too large (sum Df + Dr <= 157)");
    if (j->D != 0 && j->D < DF + Dr) return pmc_fail("pmc_joint_blocks_pre: D is smaller than the blocks and the rest together");
    if (j->D > FP_MAX_D) return pmc_fail("pmc_joint_blocks_pre: n_dim too large (D <= 157)");
    if (rest && rest->n_extended > 0 && !rest->par)
        return pmc_fail("pmc_joint_blocks_pre: factors other than uniform / normal need the parameter table (par)");
    if (DF_out) *DF_out = (int)DF;
    if (Dr_out) *Dr_out = (int)Dr;
    return 0;
}

extern "C" int pmc_joint_blocks_pre(const pmc_joint_blocks_t* j, const double* x, int64_t row_stride, int64_t col_stride,
                                    int64_t n, float* u32, double* ldj, double* rest_logp, int32_t* inside, void* stream) {
    int DF = 0, Dr = 0;
    if (int rc = pmc_joint_blocks_check(j, &DF, &Dr)) return rc;
    if (n == 0) return 0;
    if (!x || !u32 || !ldj || (Dr > 0 && !rest_logp) || !inside || n < 0 || row_stride < 0 || col_stride < 0)
        return pmc_fail("pmc_joint_blocks_pre: bad argument");
    if ((n + FP_ROWS - 1) / FP_ROWS > 0x7fffffffLL) return pmc_fail("pmc_joint_blocks_pre: too many rows for one launch");
    JointBlocksArgs a = {};
    a.n_blocks = j->n_blocks;
    for (int b = 0; b < j->n_blocks; ++b) {
        a.s[b] = *j->scaler[b];
        a.cols[b] = j->cols[b];
        a.off[b + 1] = a.off[b] + j->scaler[b]->D;
    }
    for (int b = j->n_blocks; b < PMC_JOINT_BLOCKS_MAX; ++b) a.off[b + 1] = a.off[b];
    if (j->rest) a.rest = *j->rest;
    a.rest_cols = j->rest_cols;
    a.D = j->D ? j->D : DF + Dr;
    const size_t lds = joint_blocks_lds_bytes(DF, Dr, a.D);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(joint_blocks_pre_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return pmc_fail_hip(e, "hipFuncSetAttribute(joint_blocks_pre_kernel)");
    }
    hipLaunchKernelGGL(joint_blocks_pre_kernel, dim3((unsigned)((n + FP_ROWS - 1) / FP_ROWS)), dim3(FP_THREADS), lds,
                       (hipStream_t)stream, a, x, row_stride, col_stride, n, u32, ldj, rest_logp, inside);
    return pmc_check_launch("joint_blocks_pre_kernel");
}

extern "C" int pmc_joint_blocks_post(int32_t n_blocks, const float* lp32, const double* ldj, const double* rest_logp,
                                     const int32_t* inside, double* logp, int64_t n, void* stream) {
    if (n_blocks < 1 || n_blocks > PMC_JOINT_BLOCKS_MAX) return pmc_fail("pmc_joint_blocks_post: n_blocks must lie in 1 .. 8");
    if (n == 0) return 0;
    if (!lp32 || !ldj || !inside || !logp || n < 0) return pmc_fail("pmc_joint_blocks_post: bad argument");
    if ((n + 255) / 256 > 0x7fffffffLL) return pmc_fail("pmc_joint_blocks_post: too many rows for one launch");
    hipLaunchKernelGGL(joint_blocks_post_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (int)n_blocks, lp32, ldj, rest_logp, inside, logp, n);
    return pmc_check_launch("joint_blocks_post_kernel");
}
