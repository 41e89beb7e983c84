// EM fit of a multivariate Student-t (location, scatter, degrees of freedom) to the selected rows of the pool -- what
// pocomc/student.py:53-85 sets out to do, with a root finder for nu that works (include/pocomc_amd.h: pmc_student_em).
// One EM iteration is seven launches on the caller's stream:
//   em_chol_kernel     one workgroup: packed Cholesky factor of Sigma (LDS), pivot check
//   em_delta_kernel    one lane per row: forward substitution against the factor in LDS -> delta_r
//   em_nu_kernel       one workgroup: root of f(nu) in log nu, every f an ordered reduction over delta
//   em_mom1_kernel / em_mom2_kernel / em_sigma_kernel   the partial / final structure of pool.hip's moments with
//                      w_r = (nu + D) / (nu + delta_r) formed on the fly: sum w x, sum w, sum w d d^T about the old mu
//   em_step_kernel     one workgroup: the new mu, the loop condition
// All state lives in the workspace; state->done turns every later kernel of the call into a no-op.  It is written by
// single-workgroup kernels only and read by the kernels behind them: no kernel waits for another.  Every sum has a fixed
// order (no atomics): the same rows give the same bits on every call and every device.
// pmc_student_em_weighted runs the same kernels with a weight per row (the WT = true instances): pi_r = w_r / sum w in
// place of 1 / n in every sum, rows of weight zero never read, em_weights_kernel ahead of the loop; above D = 128 its row
// pass takes 32 rows per workgroup.  The WT = false instances are the code pmc_student_em ran before the weights came.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "pmc_internal.h"

#pragma clang fp contract(off)

#define EM_CHUNKS 64          // row chunks of the weighted sums (pool.hip: MOM_CHUNKS)
#define EM_ROWS 64            // rows of one em_delta_kernel workgroup: one wavefront
#define EM_ROWS_WIDE 32       // the same above PMC_STUDENT_MAX_D (pmc_student_em_weighted): half the substitution vectors
#define EM_W_THREADS 256
#define EM_NU_THREADS 1024
#define EM_HOST_CHUNK 8       // iterations enqueued between two reads of the state

struct EmState {
    double nu, last_nu;
    int32_t iter, status, done, pad;
};

struct EmWeights {            // em_weights_kernel's record, at byte 128 of the workspace
    double sum, sum2;         // W = sum of the positive weights, sum of their squares
    int64_t positive;         // rows with w_r > 0
    int32_t bad, pad;         // a weight that is negative, NaN or inf
};

// log(a) - psi(a), a > 0, formed directly: psi(a) = psi(a + 1) - 1/a gives
//   log a - psi(a) = [log(a + 1) - psi(a + 1)] + [1/a - log1p(1/a)]      (each bracket positive)
// up to a >= 10, then the asymptotic series 1/(2a) + sum_k B_2k / (2k a^2k) to a^-16 (next term 1.8e-19 at a = 10)
__host__ __device__ static inline double log_minus_psi(double a) {
    double s = 0.0;
    while (a < 10.0) { const double r = 1.0 / a; s += r - log1p(r); a += 1.0; }
    const double r = 1.0 / a, r2 = r * r;
    const double tail = 1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 * (1.0 / 132 - r2 * (691.0 / 32760
                        - r2 * (1.0 / 12 - r2 * (3617.0 / 8160)))))));
    return s + r * (0.5 + r * tail);
}

__global__ void em_init_kernel(EmState* __restrict__ st) {
    st->nu = 20.0; st->last_nu = 0.0; st->iter = 0; st->status = PMC_STUDENT_MAX_ITER; st->done = 0; st->pad = 0;
}

// W, sum w^2, the number of positive weights and the bad-weight flag: one workgroup, thread t takes rows t, t + 256, ...
// in ascending order, then a tree over the threads
__global__ __launch_bounds__(EM_W_THREADS) void em_weights_kernel(const double* __restrict__ w, int64_t n, EmWeights* __restrict__ out) {
    __shared__ double s1[EM_W_THREADS], s2[EM_W_THREADS];
    __shared__ int64_t cnt[EM_W_THREADS];
    __shared__ int32_t bad[EM_W_THREADS];
    double a = 0.0, b = 0.0;
    int64_t c = 0;
    int32_t f = 0;
    for (int64_t r = threadIdx.x; r < n; r += EM_W_THREADS) {
        const double v = w[r];
        if (!(v >= 0.0) || !(v < __builtin_inf())) f = 1;
        else if (v > 0.0) { a += v; b += v * v; c += 1; }
    }
    s1[threadIdx.x] = a; s2[threadIdx.x] = b; cnt[threadIdx.x] = c; bad[threadIdx.x] = f;
    __syncthreads();
    for (int h = EM_W_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            s1[threadIdx.x] += s1[threadIdx.x + h]; s2[threadIdx.x] += s2[threadIdx.x + h];
            cnt[threadIdx.x] += cnt[threadIdx.x + h]; bad[threadIdx.x] |= bad[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out->sum = s1[0]; out->sum2 = s2[0]; out->positive = cnt[0]; out->bad = bad[0]; out->pad = 0; }
}

// ---------------------------------------------------------------------------------------------------------------
// Cholesky factor of Sigma, lower triangle packed by rows (L[i][j] at i (i + 1) / 2 + j), right-looking; every element
// is updated by one thread in ascending k.  A pivot <= 0 or not finite ends the fit.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void em_chol_kernel(const double* __restrict__ sigma, int D, EmState* __restrict__ st,
                                                      double* __restrict__ Lp) {
    extern __shared__ __attribute__((aligned(16))) double em_lds[];
    if (st->done) return;
    double* A = em_lds;                          // [D (D + 1) / 2]
    double* dg = A + D * (D + 1) / 2;            // [D] the factor's diagonal
    const int tid = threadIdx.x;
    for (int e = tid; e < D * D; e += 256) {
        const int i = e / D, j = e % D;
        if (j <= i) A[i * (i + 1) / 2 + j] = sigma[e];
    }
    __syncthreads();
    const int a = tid >> 4, b = tid & 15;
    for (int k = 0; k < D; ++k) {
        const double piv = A[k * (k + 1) / 2 + k];
        if (!(piv > 0.0) || !(piv < __builtin_inf())) {                 // uniform: every thread reads the same word
            if (tid == 0) { st->iter += 1; st->status = PMC_STUDENT_NOT_PD; st->done = 1; }
            return;
        }
        const double r = sqrt(piv);
        if (tid == 0) dg[k] = r;
        for (int i = k + 1 + tid; i < D; i += 256) A[i * (i + 1) / 2 + k] /= r;
        __syncthreads();
        for (int i = k + 1 + a; i < D; i += 16) {
            const double lik = A[i * (i + 1) / 2 + k];
            for (int j = k + 1 + b; j <= i; j += 16) A[i * (i + 1) / 2 + j] -= lik * A[j * (j + 1) / 2 + k];
        }
        __syncthreads();
    }
    for (int k = tid; k < D; k += 256) A[k * (k + 1) / 2 + k] = dg[k];
    __syncthreads();
    for (int e = tid; e < D * (D + 1) / 2; e += 256) Lp[e] = A[e];
    if (tid == 0) st->iter += 1;
}

// ---------------------------------------------------------------------------------------------------------------
// delta_r = |L^-1 (x_r - mu)|^2: one lane per row, the factor and mu in LDS (read at the same address by every lane),
// the lane's substitution vector y in LDS as y[j][lane].  WT: a row of weight zero is not read, its delta is 0
// ---------------------------------------------------------------------------------------------------------------
template <typename T, int ROWS, bool WT>
__global__ __launch_bounds__(ROWS) void em_delta_kernel(const T* __restrict__ x, const int64_t* __restrict__ idx,
                                                        const double* __restrict__ wts, int64_t n, int D,
                                                        const double* __restrict__ mu, const double* __restrict__ Lp,
                                                        const EmState* __restrict__ st, double* __restrict__ delta) {
    extern __shared__ __attribute__((aligned(16))) double em_lds[];
    if (st->done) return;
    const int np = D * (D + 1) / 2;
    double* L = em_lds;                          // [np]
    double* m = L + np;                          // [D]
    double* y = m + D;                           // [D][ROWS]
    const int lane = threadIdx.x;
    for (int e = lane; e < np; e += ROWS) L[e] = Lp[e];
    for (int e = lane; e < D; e += ROWS) m[e] = mu[e];
    __syncthreads();
    const int64_t r = (int64_t)blockIdx.x * ROWS + lane;
    if (r >= n) return;
    if (WT && !(wts[r] > 0.0)) { delta[r] = 0.0; return; }
    const T* row = x + (idx ? idx[r] : r) * D;
    double dl = 0.0;
    for (int i = 0; i < D; ++i) {
        const double* Li = L + i * (i + 1) / 2;
        double s0 = (double)row[i] - m[i], s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int j = 0;
        for (; j + 4 <= i; j += 4) {
            s0 -= Li[j] * y[j * ROWS + lane];
            s1 -= Li[j + 1] * y[(j + 1) * ROWS + lane];
            s2 -= Li[j + 2] * y[(j + 2) * ROWS + lane];
            s3 -= Li[j + 3] * y[(j + 3) * ROWS + lane];
        }
        for (; j < i; ++j) s0 -= Li[j] * y[j * ROWS + lane];
        const double yi = ((s0 + s1) + (s2 + s3)) / Li[i];
        y[i * ROWS + lane] = yi;
        dl += yi * yi;
    }
    delta[r] = dl;
}

// ---------------------------------------------------------------------------------------------------------------
// the nu update.  f(nu) = [log(nu/2) - psi(nu/2)] - [log((nu+D)/2) - psi((nu+D)/2)] + mean(log w - w + 1) with
// log w - w + 1 = log1p(u) - u near w = 1 and log(w) - u away from it, u = w - 1 = (D - delta) / (nu + delta).  Every
// thread holds the same root-finder state: the sum comes back through LDS, so all of them take the same branches.
// WT: sum_r pi_r (log w_r - w_r + 1) over the rows of positive weight, pi_r = wts_r / W, in place of the mean.
// ---------------------------------------------------------------------------------------------------------------
template <bool WT>
__device__ static double em_f(double nu, const double* __restrict__ delta, const double* __restrict__ wts, double W, int64_t n, int D,
                              double* part) {
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < n; e += EM_NU_THREADS) {
        if (WT && !(wts[e] > 0.0)) continue;
        const double dl = delta[e], den = nu + dl, u = ((double)D - dl) / den;     // u = w - 1
        const double v = fabs(u) < 0.5 ? log1p(u) - u : log((nu + (double)D) / den) - u;   // (a far row: w << 1, 1 + u cancels)
        if (WT) s += (wts[e] / W) * v;
        else s += v;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = EM_NU_THREADS / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    const double total = part[0];
    __syncthreads();
    return (log_minus_psi(0.5 * nu) - log_minus_psi(0.5 * (nu + D))) + (WT ? total : total / (double)n);
}

template <bool WT>
__global__ __launch_bounds__(EM_NU_THREADS) void em_nu_kernel(const double* __restrict__ delta, const double* __restrict__ wts,
                                                              const EmWeights* __restrict__ ew, int64_t n, int D,
                                                              EmState* __restrict__ st) {
    __shared__ double part[EM_NU_THREADS];
    if (st->done) return;
    const double W = WT ? ew->sum : 0.0;
    const double nu_old = st->nu;
    __syncthreads();                                   // (thread 0 writes st->nu at the end)
    double nu = 0.0;
    int status = -1;                                   // -1: the iteration goes on
    const double fhi = em_f<WT>(PMC_STUDENT_NU_HI, delta, wts, W, n, D, part);
    if (fhi != fhi) status = PMC_STUDENT_NONFINITE;
    else if (fhi >= 0.0) { nu = __builtin_inf(); status = PMC_STUDENT_NU_INF; }
    else {
        const double flo = em_f<WT>(PMC_STUDENT_NU_LO, delta, wts, W, n, D, part);
        if (flo != flo) status = PMC_STUDENT_NONFINITE;
        else if (flo <= 0.0) nu = PMC_STUDENT_NU_LO;
        else {
            // f(lo) > 0 > f(hi) in t = log nu.  Trials: the previous nu first, then the secant through the two latest
            // trials; the midpoint when the bracket has not halved over the last three trials (so it halves at least
            // that often: at most 3 * 47 trials); never closer than 3e-14 to an end of the bracket -- a one-sided
            // approach then steps past the root and closes the bracket from the other side
            double lo = log(PMC_STUDENT_NU_LO), hi = log(PMC_STUDENT_NU_HI);
            double ta = lo, fa = flo, tb = hi, fb = fhi;
            double w1 = hi - lo, w2 = w1, w3 = w1;                 // the bracket's width one, two, three trials ago
            const double t0 = log(nu_old);
            for (int ev = 0; ev < 256 && hi - lo >= 1e-13; ++ev) {
                double t;
                if (ev == 0 && t0 > lo && t0 < hi) t = t0;
                else {
                    t = fb != fa ? tb - fb * (tb - ta) / (fb - fa) : 0.5 * (lo + hi);
                    if (ev >= 3 && hi - lo > 0.5 * w3) t = 0.5 * (lo + hi);
                    if (!(t >= lo + 3e-14)) t = lo + 3e-14;
                    if (!(t <= hi - 3e-14)) t = hi - 3e-14;
                }
                const double ft = em_f<WT>(exp(t), delta, wts, W, n, D, part);
                if (ft != ft) { status = PMC_STUDENT_NONFINITE; break; }
                ta = tb; fa = fb; tb = t; fb = ft;
                w3 = w2; w2 = w1; w1 = hi - lo;
                if (ft > 0.0) lo = t;
                else if (ft < 0.0) hi = t;
                else lo = hi = t;
            }
            nu = exp(0.5 * (lo + hi));
        }
    }
    if (threadIdx.x == 0) {
        if (status != PMC_STUDENT_NONFINITE) { st->last_nu = nu_old; st->nu = nu; }
        if (status >= 0) { st->status = status; st->done = 1; }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// weighted sums with w_r = (nu + D) / (nu + delta_r): pool.hip's mom1 / mom2 partials and their ordered finals.
// WT: w_r = pi_r (nu + D) / (nu + delta_r), and a row of weight zero adds nothing and is not read
// ---------------------------------------------------------------------------------------------------------------
template <typename T, bool WT>
__global__ __launch_bounds__(256) void em_mom1_kernel(const T* __restrict__ x, const int64_t* __restrict__ idx,
                                                      const double* __restrict__ wts, const EmWeights* __restrict__ ew,
                                                      const double* __restrict__ delta, const EmState* __restrict__ st, int64_t n,
                                                      int D, double* __restrict__ part /* [EM_CHUNKS][D + 1] */) {
    if (st->done) return;
    const double nu = st->nu, num = nu + (double)D;
    const double W = WT ? ew->sum : 0.0;
    const int c = blockIdx.x;
    const int64_t per = (n + EM_CHUNKS - 1) / EM_CHUNKS;
    const int64_t lo = c * per, hi = lo + per < n ? lo + per : n;
    for (int j = threadIdx.x; j < D + 1; j += 256) {
        double s = 0.0;
        for (int64_t r = lo; r < hi; ++r) {
            if (WT && !(wts[r] > 0.0)) continue;
            const double wr = WT ? (wts[r] / W) * (num / (nu + delta[r])) : num / (nu + delta[r]);
            if (j < D) { const int64_t row = idx ? idx[r] : r; s += wr * (double)x[row * D + j]; }
            else s += wr;
        }
        part[(size_t)c * (D + 1) + j] = s;
    }
}

// grid (EM_CHUNKS, tiles_i * tiles_j): a 16 x 16 tile of sum w d d^T over one row chunk, d = x - mu (the old mu)
template <typename T, bool WT>
__global__ __launch_bounds__(256) void em_mom2_kernel(const T* __restrict__ x, const int64_t* __restrict__ idx,
                                                      const double* __restrict__ wts, const EmWeights* __restrict__ ew,
                                                      const double* __restrict__ delta, const EmState* __restrict__ st,
                                                      const double* __restrict__ mu, int64_t n, int D,
                                                      double* __restrict__ part /* [EM_CHUNKS][D][D] */) {
    __shared__ double xi[16][17], xj[16][17], wr[16];
    if (st->done) return;
    const double nu = st->nu, num = nu + (double)D;
    const double W = WT ? ew->sum : 0.0;
    const int c = blockIdx.x, nt = (D + 15) / 16;
    const int ti = blockIdx.y / nt, tj = blockIdx.y % nt;
    if (tj < ti) return;                                            // symmetric: upper tiles only
    const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
    const int i = 16 * ti + a, j = 16 * tj + b;
    const int64_t per = (n + EM_CHUNKS - 1) / EM_CHUNKS;
    const int64_t lo = c * per, hi = lo + per < n ? lo + per : n;
    double s = 0.0;
    for (int64_t r0 = lo; r0 < hi; r0 += 16) {
        {
            const int64_t r = r0 + a;
            double vi = 0.0, vj = 0.0;
            if (r < hi && !(WT && !(wts[r] > 0.0))) {
                const int64_t row = idx ? idx[r] : r;
                const int ci = 16 * ti + b, cj = 16 * tj + b;
                if (ci < D) vi = (double)x[row * D + ci] - mu[ci];
                if (cj < D) vj = (double)x[row * D + cj] - mu[cj];
                if (b == 0) wr[a] = WT ? (wts[r] / W) * (num / (nu + delta[r])) : num / (nu + delta[r]);
            } else if (b == 0) wr[a] = 0.0;
            xi[a][b] = vi; xj[a][b] = vj;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) s += (wr[k] * xi[k][a]) * xj[k][b];
        __syncthreads();
    }
    if (i < D && j < D) part[((size_t)c * D + i) * D + j] = s;
}

// Sigma = sum_c part / n (WT: the weights pi_r are in the partials already)
template <bool WT>
__global__ __launch_bounds__(256) void em_sigma_kernel(const double* __restrict__ part, const EmState* __restrict__ st, int64_t n,
                                                       int D, double* __restrict__ sigma) {
    if (st->done) return;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < D * D; e += gridDim.x * 256) {
        const int i = e / D, j = e % D;
        const int ii = i <= j ? i : j, jj = i <= j ? j : i;           // the upper triangle was computed
        double s = 0.0;
        for (int c = 0; c < EM_CHUNKS; ++c) s += part[((size_t)c * D + ii) * D + jj];
        sigma[e] = WT ? s : s / (double)n;
    }
}

// mu = sum w x / sum w, then the loop condition of the iteration that ends here
__global__ __launch_bounds__(128) void em_step_kernel(const double* __restrict__ part, int D, double tol, int max_iter,
                                                      EmState* __restrict__ st, double* __restrict__ mu) {
    if (st->done) return;
    double sw = 0.0;
    for (int c = 0; c < EM_CHUNKS; ++c) sw += part[(size_t)c * (D + 1) + D];
    for (int j = threadIdx.x; j < D; j += 128) {
        double s = 0.0;
        for (int c = 0; c < EM_CHUNKS; ++c) s += part[(size_t)c * (D + 1) + j];
        mu[j] = s / sw;
    }
    __syncthreads();                                   // (every thread has read st->done)
    if (threadIdx.x == 0) {
        const bool conv = !(fabs(st->last_nu - st->nu) > tol);
        if (conv || st->iter >= max_iter) {
            st->status = st->nu == PMC_STUDENT_NU_LO ? PMC_STUDENT_LOWER_CLAMP : conv ? PMC_STUDENT_CONVERGED : PMC_STUDENT_MAX_ITER;
            st->done = 1;
        }
    }
}

// workspace: state (the weight record at byte 128) | packed factor | delta [n] | mom1 partials | mom2 partials
static inline size_t em_align(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" int64_t pmc_student_em_workspace_bytes(int64_t n, int32_t D) {
    if (n < 1 || D < 1) return 0;
    const size_t d = (size_t)D;
    return (int64_t)(256 + em_align(8 * d * (d + 1) / 2) + em_align(8 * (size_t)n) + em_align(8 * EM_CHUNKS * (d + 1))
                     + em_align(8 * EM_CHUNKS * d * d));
}

extern "C" int64_t pmc_student_em_weighted_workspace_bytes(int64_t n, int32_t D) { return pmc_student_em_workspace_bytes(n, D); }

// WT = false: pmc_student_em (wts == NULL, result [4]); WT = true: pmc_student_em_weighted (idx == NULL, result [6])
template <typename T, bool WT>
static int em_run(const char* name, const T* x, const int64_t* idx, const double* wts, int64_t n, int D, double* mu, double* sigma,
                  double tol, int max_iter, double* result, char* ws, hipStream_t st) {
    const size_t d = (size_t)D;
    EmState* state = (EmState*)ws;
    const EmWeights* ew = (const EmWeights*)(ws + 128);
    double* Lp = (double*)(ws + 256);
    double* delta = (double*)((char*)Lp + em_align(8 * d * (d + 1) / 2));
    double* p1 = (double*)((char*)delta + em_align(8 * (size_t)n));
    double* p2 = (double*)((char*)p1 + em_align(8 * EM_CHUNKS * (d + 1)));
    const bool wide = WT && D > PMC_STUDENT_MAX_D;         // 32 rows per workgroup: 140,672 bytes of LDS at D = 157
    const size_t lds_chol = 8 * (d * (d + 1) / 2 + d);
    const size_t lds_delta = 8 * (d * (d + 1) / 2 + d + d * (size_t)(wide ? EM_ROWS_WIDE : EM_ROWS));
    EmWeights hw = {};
    int reads = 0;
    if (WT) {
        hipLaunchKernelGGL(em_weights_kernel, dim3(1), dim3(EM_W_THREADS), 0, st, wts, n, (EmWeights*)(ws + 128));
        int rc = pmc_check_launch(name);
        if (rc) return rc;
        hipError_t e = hipMemcpyAsync(&hw, ew, sizeof(EmWeights), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return pmc_fail_hip(e, "pmc_student_em_weighted: reading the weight record");
        ++reads;
        if (hw.bad) return pmc_fail("pmc_student_em_weighted: weights must be finite and non-negative");
        if (hw.positive <= (int64_t)D) return pmc_fail("pmc_student_em_weighted: needs more rows of positive weight than dimensions");
    }
    if (lds_chol > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(em_chol_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_chol);
        if (e != hipSuccess) return pmc_fail_hip(e, "hipFuncSetAttribute(em_chol_kernel)");
    }
    void (*delta_kernel)(const T*, const int64_t*, const double*, int64_t, int, const double*, const double*, const EmState*, double*)
        = em_delta_kernel<T, EM_ROWS, WT>;
    if constexpr (WT) if (wide) delta_kernel = em_delta_kernel<T, EM_ROWS_WIDE, true>;
    const int rows = wide ? EM_ROWS_WIDE : EM_ROWS;
    if (lds_delta > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(delta_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_delta);
        if (e != hipSuccess) return pmc_fail_hip(e, "hipFuncSetAttribute(em_delta_kernel)");
    }
    const int nt = (D + 15) / 16;
    // (the lower tiles of em_mom2_kernel write nothing and em_sigma_kernel reads the upper triangle only: no memset)
    hipLaunchKernelGGL(em_init_kernel, dim3(1), dim3(1), 0, st, state);
    EmState h = {};
    for (int it = 0; it < max_iter && !h.done;) {
        for (int k = 0; k < EM_HOST_CHUNK && it < max_iter; ++k, ++it) {
            hipLaunchKernelGGL(em_chol_kernel, dim3(1), dim3(256), lds_chol, st, (const double*)sigma, D, state, Lp);
            hipLaunchKernelGGL(delta_kernel, dim3((unsigned)((n + rows - 1) / rows)), dim3(rows), lds_delta, st, x, idx, wts, n, D,
                               (const double*)mu, (const double*)Lp, (const EmState*)state, delta);
            hipLaunchKernelGGL(em_nu_kernel<WT>, dim3(1), dim3(EM_NU_THREADS), 0, st, (const double*)delta, wts, ew, n, D, state);
            hipLaunchKernelGGL((em_mom1_kernel<T, WT>), dim3(EM_CHUNKS), dim3(256), 0, st, x, idx, wts, ew, (const double*)delta,
                               (const EmState*)state, n, D, p1);
            hipLaunchKernelGGL((em_mom2_kernel<T, WT>), dim3(EM_CHUNKS, nt * nt), dim3(256), 0, st, x, idx, wts, ew, (const double*)delta,
                               (const EmState*)state, (const double*)mu, n, D, p2);
            hipLaunchKernelGGL(em_sigma_kernel<WT>, dim3((D * D + 255) / 256), dim3(256), 0, st, (const double*)p2, (const EmState*)state,
                               n, D, sigma);
            hipLaunchKernelGGL(em_step_kernel, dim3(1), dim3(128), 0, st, (const double*)p1, D, tol, max_iter, state, mu);
        }
        int rc = pmc_check_launch(name);
        if (rc) return rc;
        hipError_t e = hipMemcpyAsync(&h, state, sizeof(EmState), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return pmc_fail_hip(e, "pmc_student_em: reading the state");
        ++reads;
    }
    if (!h.done) return pmc_fail("pmc_student_em: the fit did not end (internal error)");
    result[0] = h.nu; result[1] = (double)h.iter; result[2] = (double)h.status; result[3] = (double)reads;
    if (WT) { result[4] = (double)hw.positive; result[5] = hw.sum * hw.sum / hw.sum2; }
    return 0;
}

// x: f64 [*][D] (x32 == NULL) or f32 (x32 != NULL); idx i64 [n] or NULL (rows 0..n-1); result: host f64 [4]
extern "C" int pmc_student_em(const double* x, const float* x32, const int64_t* idx, int64_t n, int32_t D, double* mu_io,
                              double* sigma_io, double tol, int32_t max_iter, double* result, void* workspace,
                              int64_t workspace_bytes, void* stream) {
    if ((!x && !x32) || !mu_io || !sigma_io || !result || !workspace || n < 1 || D < 1 || max_iter < 1 || !(tol >= 0.0))
        return pmc_fail("pmc_student_em: bad argument");
    if (D > PMC_STUDENT_MAX_D) return pmc_fail("pmc_student_em: D > 128 (the packed Cholesky factor and 64 rows' substitution vectors share the LDS)");
    if (n <= D) return pmc_fail("pmc_student_em: needs more rows than dimensions");
    if (workspace_bytes < pmc_student_em_workspace_bytes(n, D)) return pmc_fail("pmc_student_em: workspace too small");
    if (x32) return em_run<float, false>("pmc_student_em", x32, idx, nullptr, n, (int)D, mu_io, sigma_io, tol, (int)max_iter, result,
                                         (char*)workspace, (hipStream_t)stream);
    return em_run<double, false>("pmc_student_em", x, idx, nullptr, n, (int)D, mu_io, sigma_io, tol, (int)max_iter, result,
                                 (char*)workspace, (hipStream_t)stream);
}

// the same fit with a weight per row: x rows 0..n-1, w f64 [n] >= 0 (device); result: host f64 [6]
extern "C" int pmc_student_em_weighted(const double* x, const float* x32, const double* w, int64_t n, int32_t D, double* mu_io,
                                       double* sigma_io, double tol, int32_t max_iter, double* result, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
    if ((!x && !x32) || !w || !mu_io || !sigma_io || !result || !workspace || n < 1 || D < 1 || max_iter < 1 || !(tol >= 0.0))
        return pmc_fail("pmc_student_em_weighted: bad argument");
    if (D > PMC_STUDENT_W_MAX_D) return pmc_fail("pmc_student_em_weighted: D > 157 (the widest MCMC step)");
    if (n <= D) return pmc_fail("pmc_student_em_weighted: needs more rows of positive weight than dimensions");
    if (workspace_bytes < pmc_student_em_weighted_workspace_bytes(n, D)) return pmc_fail("pmc_student_em_weighted: workspace too small");
    if (x32) return em_run<float, true>("pmc_student_em_weighted", x32, nullptr, w, n, (int)D, mu_io, sigma_io, tol, (int)max_iter, result,
                                        (char*)workspace, (hipStream_t)stream);
    return em_run<double, true>("pmc_student_em_weighted", x, nullptr, w, n, (int)D, mu_io, sigma_io, tol, (int)max_iter, result,
                                (char*)workspace, (hipStream_t)stream);
}
