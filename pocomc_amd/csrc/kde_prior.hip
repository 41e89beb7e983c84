// A weighted Gaussian kernel density estimate of M samples with ONE shared bandwidth matrix H on dim columns of x, and an
// optional table of scipy factors on others (pocomc_amd/prior.py: KDEPrior, and the KDE blocks of JointPrior):
//   log p(x) = start + log sum_m w_m N(x_cols; s_m, H),   start = base[r], the table's sum, or nothing.
// The shared H makes this another problem than gauss_mix_prior.hip's: a row is whitened ONCE, y = Linv (x - center), the
// samples arrive whitened from the host, t_m = Linv (s_m - center), and a kernel of the estimate is dim subtractions, dim
// squares and one exp: an n x M streaming log-sum-exp in two passes, float64 VALU, one launch, one pass over x.  The order
// of every addition that the statement fixes is fixed (include/pocomc_amd.h, tests/kde_model.py) and nothing is contracted
// into an FMA: the y_i and every e_m of a row are the numpy model's bits; the sum of the exps is split in eight slices.
#include "gauss_body.h"
#include "prior_body.h"

#pragma clang fp contract(off)

// What the kernel takes of the host's pmc_kde_t: everything by value.
struct KdeArgs {
    const int32_t* cols;
    const double* center;
    const double* linv;
    const double* t;
    const double* logw;
    double logc;
    int32_t n_samples;
    int32_t D;
    int32_t Dr;                                    // 0: no table
    pmc_prior_t rest;
    const int32_t* rest_cols;
};

// The x tile, the wavefronts' partial maxima and partial sums, one flag per row:
// 64 (D | 1) 8 + 2 * 8 * 64 * 8 + 256 bytes; 80384 + 8192 + 256 = 88832 at D = 157.
static inline size_t kde_lds_bytes(int D) {
    return ((size_t)FP_ROWS * (D | 1) + 2 * (size_t)GP_WAVES * FP_ROWS) * sizeof(double) + FP_ROWS * sizeof(int);
}

// e_m of the lane's row for sample m: q = ((0.0 + (y_0 - t_m0)^2) + (y_1 - t_m1)^2) + ..., e = -0.5 q + logw_m.  t and logw
// sit at addresses the wavefront shares: scalar loads.
template <int K>
__device__ __forceinline__ double kde_e(const double (&y)[K], gp_f64 t, gp_f64 logw, int m) {
    gp_f64 tm = t + (int64_t)m * K;
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const double df = y[j] - tm[j];
        q = q + df * df;
    }
    return -0.5 * q + logw[m];
}

// gauss_blocks_kernel's tile and stride contract (gauss_load_tile: 64 rows of all D columns through LDS, the two coalesced
// layouts), lane = row of the tile, wavefront w = tid / 64.  K = dim is a template argument: the row's y stays in K
// registers, every loop over j is unrolled and no register array is indexed at run time.
//   0. every table column's x becomes its factor's term (wavefront w takes the factors w, w + 8, ...); a row with a block or
//      table x that is not finite or a table term that is NaN is marked in rowin, and so are the rows of a tile with a column
//      outside [0, D), which is not followed.
//   1. EVERY wavefront whitens its lane's row for itself: d_j = x[cols[j]] - center_j, y_i = ((0.0 + Linv[i,0] d_0) +
//      Linv[i,1] d_1) + ... -- K (K + 1) / 2 <= 136 products, nothing next to M kernels, and no barrier or LDS round trip
//      to hand y to the other seven wavefronts.  The block's columns of the tile are only read.
//   2. the M samples are cut in eight contiguous slices of ceil(M / 8), wavefront w takes slice w (the cut depends on M
//      alone: a row's bits do not depend on n or on its place).  Pass 1: the slice's max_m e_m into PM[w][row]; behind a
//      barrier every lane takes mx = max_w PM[w][row] (a maximum has no order).
//   3. Pass 2: the slice's e_m again (the same instructions, the same bits), s_w = (0.0 + exp(e_m0 - mx)) + ... in m order,
//      into PS[w][row]; behind a barrier one lane per row adds s = ((s_0 + s_1) + ...) + s_7 in wavefront order (an empty
//      slice gives 0.0), v = (mx + log s) - logc, logp = start + v.  mx = -inf: the row is -inf and the differences are
//      formed against 0.0 instead (exp(-inf) = 0, no NaN is made).
// The bits of a row depend on its values and the descriptor alone.  Every barrier is reached by every thread: the trip
// counts depend on the descriptor alone, and lanes behind the last row compute on what the tile holds and store nothing.
template <int K>
__global__ __launch_bounds__(FP_THREADS) void kde_kernel(KdeArgs a, const double* __restrict__ x, int64_t row_stride,
                                                         int64_t col_stride, int64_t n, const double* base, double* logp) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int M = a.n_samples, D = a.D, Dr = a.Dr, LD = D | 1;
    double* T = sm;                                                       // [FP_ROWS][LD]
    double* PM = T + (size_t)FP_ROWS * LD;                                // [GP_WAVES][FP_ROWS]
    double* PS = PM + GP_WAVES * FP_ROWS;                                 // [GP_WAVES][FP_ROWS]
    int* rowin = reinterpret_cast<int*>(PS + GP_WAVES * FP_ROWS);         // [FP_ROWS]
    const int tid = threadIdx.x;
    const int r = tid & (FP_ROWS - 1);
    const int w = __builtin_amdgcn_readfirstlane(tid / FP_ROWS);
    const int64_t row0 = (int64_t)blockIdx.x * FP_ROWS;
    const int rows = (int)min((int64_t)FP_ROWS, n - row0);
    const gp_i32 cols = (gp_i32)a.cols;
    const gp_f64 tw = (gp_f64)a.t, logw = (gp_f64)a.logw;
    if (tid < FP_ROWS) rowin[tid] = 1;
    gauss_load_tile(T, x, row_stride, col_stride, row0, rows, D, LD, tid);
    __syncthreads();
    double* Tr = T + r * LD;
    const bool live = r < rows;
    // 0. the table's terms, and the rows the estimate has no value for
    for (int j = w; j < K; j += GP_WAVES) {
        const int c = cols[j];
        const bool col_ok = (unsigned)c < (unsigned)D;
        if (!live) continue;
        if (!col_ok || !isfinite(Tr[c])) rowin[r] = 0;
    }
    for (int m = w; m < Dr; m += GP_WAVES) {
        const int c = a.rest_cols[m];
        const bool col_ok = (unsigned)c < (unsigned)D;
        if (!live) continue;
        if (!col_ok) { rowin[r] = 0; continue; }
        const double xv = Tr[c];
        const double term = prior_term_any(a.rest, m, xv);
        Tr[c] = term;
        if (!isfinite(xv) || isnan(term)) rowin[r] = 0;
    }
    // 1. y = Linv (x - center), the row's, in registers
    double y[K];
    {
        const gp_f64 center = (gp_f64)a.center, linv = (gp_f64)a.linv;
        double d[K];
#pragma unroll
        for (int j = 0; j < K; ++j) d[j] = Tr[gauss_col(cols, j, D)] - center[j];
#pragma unroll
        for (int i = 0; i < K; ++i) {
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j <= i; ++j) acc = acc + linv[(i * (i + 1)) / 2 + j] * d[j];
            y[i] = acc;
        }
    }
    // 2. the slice's maximum, then the row's
    const int chunk = (M + GP_WAVES - 1) / GP_WAVES;
    const int m0 = min(M, w * chunk), m1 = min(M, m0 + chunk);
    double mx = -INFINITY;
#pragma unroll 4
    for (int m = m0; m < m1; ++m) {
        const double e = kde_e<K>(y, tw, logw, m);
        mx = e > mx ? e : mx;
    }
    PM[w * FP_ROWS + r] = mx;
    __syncthreads();
    mx = PM[r];
#pragma unroll
    for (int u = 1; u < GP_WAVES; ++u) {
        const double p = PM[u * FP_ROWS + r];
        mx = p > mx ? p : mx;
    }
    // 3. the slice's sum, then the row's value
    const double ref = mx == -INFINITY ? 0.0 : mx;
    double s = 0.0;
#pragma unroll 2
    for (int m = m0; m < m1; ++m) s = s + exp(kde_e<K>(y, tw, logw, m) - ref);
    PS[w * FP_ROWS + r] = s;
    __syncthreads();
    if (tid < rows) {
        double v = -INFINITY;
        if (mx != -INFINITY) {
            double st = PS[tid];
#pragma unroll
            for (int u = 1; u < GP_WAVES; ++u) st = st + PS[u * FP_ROWS + tid];
            v = (mx + log(st)) - a.logc;
        }
        if (base) {
            v = base[row0 + tid] + v;
        } else if (Dr > 0) {
            double lp = 0.0;
            for (int mm = 0; mm < Dr; ++mm) lp += Tr[gauss_col((gp_i32)a.rest_cols, mm, D)];
            v = lp + v;
        }
        logp[row0 + tid] = (rowin[tid] && isfinite(v)) ? v : -INFINITY;
    }
}

template <int K>
static int kde_launch(const KdeArgs& a, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,
                      const double* base, double* logp, void* stream) {
    const size_t lds = kde_lds_bytes(a.D);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kde_kernel<K>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return pmc_fail_hip(e, "hipFuncSetAttribute(kde_kernel)");
    }
    const dim3 grid((unsigned)((n + FP_ROWS - 1) / FP_ROWS)), block(FP_THREADS);
    hipLaunchKernelGGL(kde_kernel<K>, grid, block, lds, (hipStream_t)stream, a, x, row_stride, col_stride, n, base, logp);
    return pmc_check_launch("kde_kernel");
}

extern "C" int pmc_kde_logpdf(const pmc_kde_t* g, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,
                              const double* base, double* logp, void* stream) {
#define KDE_FAIL(text) return pmc_fail("pmc_kde_logpdf: " text)
    if (!g) KDE_FAIL("bad descriptor");
    if (!g->cols || !g->center || !g->linv || !g->t || !g->logw) KDE_FAIL("bad KDE descriptor (a NULL array)");
    if (g->n_samples < 1 || g->n_samples > PMC_KDE_MAX_SAMPLES) KDE_FAIL("n_samples must lie in 1 .. 65536");
    if (g->dim < 1 || g->dim > PMC_KDE_MAX_DIM) KDE_FAIL("dim must lie in 1 .. 16");
    if (g->D > FP_MAX_D) KDE_FAIL("n_dim too large (D <= 157)");
    const pmc_prior_t* rest = g->rest;
    if ((rest == nullptr) != (g->rest_cols == nullptr)) KDE_FAIL("rest and rest_cols go together (both, or both NULL)");
    if (rest && (!rest->family || !rest->loc || !rest->scale || rest->n_extended < 0 || rest->D < 1))
        KDE_FAIL("bad prior descriptor");
    const int64_t Dr = rest ? rest->D : 0;
    if ((int64_t)g->dim + Dr > g->D) KDE_FAIL("the KDE block and the rest have more columns than x (D)");
    if (rest && rest->n_extended > 0 && !rest->par)
        KDE_FAIL("factors other than uniform / normal need the parameter table (par)");
    if (base && rest) KDE_FAIL("base and rest exclude each other");
    if (n == 0) return 0;
    if (!x || !logp) KDE_FAIL("bad argument (a NULL x or logp)");
    if (n < 0 || row_stride < 0 || col_stride < 0) KDE_FAIL("bad argument (a negative count or stride)");
    if ((n + FP_ROWS - 1) / FP_ROWS > 0x7fffffffLL) KDE_FAIL("too many rows for one launch");
#undef KDE_FAIL
    KdeArgs a = {};
    a.cols = g->cols;
    a.center = g->center;
    a.linv = g->linv;
    a.t = g->t;
    a.logw = g->logw;
    a.logc = g->logc;
    a.n_samples = g->n_samples;
    a.D = g->D;
    a.Dr = (int32_t)Dr;
    if (rest) a.rest = *rest;
    a.rest_cols = g->rest_cols;
    switch (g->dim) {
#define KDE_CASE(K) case K: return kde_launch<K>(a, x, row_stride, col_stride, n, base, logp, stream);
    KDE_CASE(1) KDE_CASE(2) KDE_CASE(3) KDE_CASE(4) KDE_CASE(5) KDE_CASE(6) KDE_CASE(7) KDE_CASE(8)
    KDE_CASE(9) KDE_CASE(10) KDE_CASE(11) KDE_CASE(12) KDE_CASE(13) KDE_CASE(14) KDE_CASE(15) KDE_CASE(16)
#undef KDE_CASE
    }
    return pmc_fail("pmc_kde_logpdf: dim must lie in 1 .. 16");
}
