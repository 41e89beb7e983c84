// Element-wise pieces of the scaler (pocomc/scaler.py) and of Prior.logpdf (pocomc/prior.py), shared by the scaler
// kernels (mcmc_kernels.hip) and by the epilogue of the flow-inverse sweeps (maf_inverse_tri4.hip), which applies the
// scaler to its 16 walkers while they are still in LDS: one launch and one global round trip less per MCMC step.
// float64 in numpy's operation order, no FMA contraction: both users produce the same bits.
#ifndef PMC_SCALER_BODY_H
#define PMC_SCALER_BODY_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/pocomc_amd.h"

#pragma clang fp contract(off)

// ===========================================================================
// scaler: Reparameterize.inverse / forward (scaler.py:180-226, :293-425)
// ===========================================================================
#define LOG_SQRT_2PI 0.91893853320467267   // np.log(np.sqrt(2.0*np.pi))
#define SQRT2 1.4142135623730951           // np.sqrt(2.0)

// numpy's pairwise summation (umath loops, PW_BLOCKSIZE = 128), so that the row sum of
// the Jacobian terms (scaler.py:270) is accumulated in numpy's order
__device__ __forceinline__ double np_pairwise_leaf(const double* a, int n) {   // n <= 128
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i;
    for (i = 8; i < n - (n % 8); i += 8) {
        r0 += a[i + 0]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < n; ++i) res += a[i];
    return res;
}

// numpy splits n > 128 in halves (first half rounded down to a multiple of 8), recursively;
// three explicit levels cover n <= 1024 without a device-side call stack
template <int LEVEL>
__device__ __forceinline__ double np_pairwise_sum_l(const double* a, int n) {
    if (n <= 128) return np_pairwise_leaf(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    if constexpr (LEVEL > 0) return np_pairwise_sum_l<LEVEL - 1>(a, n2) + np_pairwise_sum_l<LEVEL - 1>(a + n2, n - n2);
    else return np_pairwise_leaf(a, n2) + np_pairwise_leaf(a + n2, n - n2);
}

__device__ __forceinline__ double np_pairwise_sum(const double* a, int n) { return np_pairwise_sum_l<2>(a, n); }

// The two families the epilogues of the fused sweeps evaluate: pmc_prior_t up to `reserved` (a prior with a factor of
// another family takes the scaler launch of its own, prior_body.h)
struct pmc_prior_un_t {
    const int32_t* family;
    const double* loc;
    const double* scale;
    int32_t D;
    int32_t reserved;
};

// What an element needs of its feature j: the scaler's per-feature constants and the feature's factor of the prior.  The
// users fetch it once per feature -- every field requested before the first is waited for -- and keep it in registers
// over the feature's elements: loaded where they are used, under the branches on the kind and the family, the fields
// came as four to five L2 round trips in a row for every element.
struct ScalerFeat {
    double mu, sigma;                              // affine part (s.scale)
    double low, high, log_width;
    double loc, pscale, log_pscale;                // the prior's factor: loc, scale and log(scale) (uniform: the value inside
                                                   // the support is its negative; normal: the term subtracted)
    int kind, bc, family;
};

// The loads alone.  A field the descriptors do not have (mu / sigma without the affine part, bc == NULL, no prior) is read
// from an array they do have and never used: a request under a branch would be waited for where the branch joins.
// pr: pmc_prior_t / pmc_prior_un_t, or NULL
template <class P>
__device__ __forceinline__ void scaler_feat_request(ScalerFeat& f, const pmc_scaler_t& s, const P* pr, int j) {
    const double* mu = s.scale ? s.mu : s.low;
    const double* sigma = s.scale ? s.sigma : s.low;
    const int32_t* bc = s.bc ? s.bc : s.kind;
    const double* loc = pr ? pr->loc : s.low;
    const double* pscale = pr ? pr->scale : s.low;
    const int32_t* family = pr ? pr->family : s.kind;
    f.mu = mu[j]; f.sigma = sigma[j];
    f.low = s.low[j]; f.high = s.high[j]; f.log_width = s.log_width[j];
    f.loc = loc[j]; f.pscale = pscale[j];
    f.kind = s.kind[j]; f.bc = bc[j]; f.family = family[j];
    f.log_pscale = 0.0;
}
// what is computed from the fields (waits for them): log(scale) of the prior's factor, once per feature instead of once
// per element -- the same device log of the same value
__device__ __forceinline__ void scaler_feat_finish(ScalerFeat& f, const pmc_scaler_t& s, bool have_prior) {
    if (!s.bc) f.bc = 0;
    if (have_prior) f.log_pscale = log(f.pscale);
}

// bounded <- unbounded for one element; t is the (affine-transformed) input.  scaler.py:329-425
__device__ __forceinline__ void bound_inverse(const ScalerFeat& f, int logit, double t, double& x, double& J) {
    if (f.kind == 0) { x = t; J = 0.0; }
    else if (f.kind == 1) { x = exp(t) + f.low; J = t; }
    else if (f.kind == 2) { x = f.high - exp(t); J = t; }
    else {
        const double w = f.high - f.low;
        if (logit) {
            // p = exp(-logaddexp(0, -t))
            const double mt = -t;
            double lae;
            if (mt == 0.0) lae = 0.6931471805599453;
            else if (0.0 - mt > 0.0) lae = 0.0 + log1p(exp(-(0.0 - mt)));
            else lae = mt + log1p(exp(0.0 - mt));
            const double p = exp(-lae);
            x = p * w + f.low;
            J = (f.log_width + log(p)) + log(1.0 - p);
        } else {
            const double p = (erf(t / SQRT2) + 1.0) / 2.0;
            x = p * w + f.low;
            J = (f.log_width + (-(t * t) / 2.0)) - LOG_SQRT_2PI;
        }
    }
}

// unbounded <- bounded (scaler.py:228-247, :315-400), then the affine part (:273-289)
__device__ __forceinline__ double bound_forward(const ScalerFeat& f, int logit, int scale, double x) {
    double u;
    if (f.kind == 0) u = x;
    else if (f.kind == 1) u = log(x - f.low);
    else if (f.kind == 2) u = log(f.high - x);
    else {
        const double p = (x - f.low) / (f.high - f.low);
        if (logit) u = log(p / (1.0 - p));
        else u = SQRT2 * erfinv(2.0 * p - 1.0);
    }
    if (scale) u = (u - f.mu) / f.sigma;
    return u;
}
// (one element, the feature's constants from the descriptor: scaler_forward_kernel)
__device__ __forceinline__ double bound_forward(const pmc_scaler_t& s, int j, double x) {
    ScalerFeat f;
    scaler_feat_request(f, s, (const pmc_prior_un_t*)nullptr, j);
    return bound_forward(f, s.logit, s.scale, x);
}

// periodic wrap / reflective fold (scaler.py:109-157).  The reference loops "while
// outside"; a non-finite x would never leave that loop, the device bounds it.
__device__ __forceinline__ double apply_bc(const ScalerFeat& f, double x) {
    const int bc = f.bc;
    if (bc == 0) return x;
    const double lo = f.low, hi = f.high;
    {
        if (bc & 1) {
            for (int it = 0; it < 4096 && x > hi; ++it) x = lo + x - hi;
            for (int it = 0; it < 4096 && x < lo; ++it) x = hi + x - lo;
        }
        if (bc & 2) {
            for (int it = 0; it < 4096 && x > hi; ++it) x = hi - x + hi;
            for (int it = 0; it < 4096 && x < lo; ++it) x = lo + lo - x;
        }
    }
    return x;
}

// one uniform / normal factor of Prior.logpdf (pocomc/prior.py:70-100), shared by prior_logpdf_kernel, the scaler kernel
// and the epilogues of the fused sweeps
__device__ __forceinline__ double prior_term(const ScalerFeat& f, double xv) {
    if (f.family == PMC_PRIOR_UNIFORM) {
        // scipy uniform(loc, scale).logpdf: -log(scale) on [loc, loc+scale], -inf outside
        return (xv >= f.loc && xv <= f.loc + f.pscale) ? -f.log_pscale : -INFINITY;
    }
    // scipy norm(loc, scale).logpdf: _norm_logpdf((x-loc)/scale) - log(scale)
    const double z = (xv - f.loc) / f.pscale;
    return (-(z * z) / 2.0 - LOG_SQRT_2PI) - f.log_pscale;
}
// (the factor's constants from the descriptor; P: pmc_prior_t or pmc_prior_un_t)
template <class P>
__device__ __forceinline__ double prior_term(const P& pr, int j, double xv) {
    ScalerFeat f;
    f.loc = pr.loc[j]; f.pscale = pr.scale[j]; f.family = pr.family[j];
    f.log_pscale = log(f.pscale);
    return prior_term(f, xv);
}


// one element of the scaler inverse: u in; u (re-derived from x when boundary conditions apply), x and the Jacobian term J
// out.  Shared by scaler_inverse_kernel and the epilogue of the fused sweeps.
__device__ __forceinline__ void scaler_element(const pmc_scaler_t& s, const ScalerFeat& f, double& u, double& x, double& J) {
    double t = s.scale ? f.mu + f.sigma * u : u;
    bound_inverse(f, s.logit, t, x, J);
    if (s.bc) {
        // mcmc.py:94-97: wrap x, re-derive u from it, invert again
        x = apply_bc(f, x);
        u = bound_forward(f, s.logit, s.scale, x);
        t = s.scale ? f.mu + f.sigma * u : u;
        bound_inverse(f, s.logit, t, x, J);
    }
}

// The completion word of a hand-over (pmc_handover_t.done_flag, pinned host memory: the host spins on it instead of going
// through the runtime), behind a workgroup's last store; every thread of the workgroup calls it (it synchronises).
// Every thread waits for the acknowledgement of its own stores (agent-scope release: pinned host memory is not cached on
// the device, so there is nothing to write back), the workgroup draws a ticket (agent-scope acq_rel), the last one moves
// the row count and publishes the word with a system-scope release.  A __threadfence_system() in the fence's place made
// every one of the ~400 workgroups write back and invalidate the whole L2: 12 us of the launch (timing-only builds of this
// file), 6 us in scripts/micro/pcie_store.hip, which also checks that the host never sees the word before the data (0 stale
// words in 8000 launches x 208 k words with either fence).
// stamps: measurement only (ScalerEpi::stamps), slot 5 between the barrier and the ticket; NULL elsewhere.
__device__ __forceinline__ void handover_complete(const pmc_handover_t& h, long long* stamps, int tid) {
    if (!h.done_flag) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (stamps && tid == 0) stamps[blockIdx.x * 8 + 5] = wall_clock64();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(h.done_ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (t == gridDim.x - 1) {
            *h.done_ticket = 0u;
            if (h.bad_count && h.bad_flag) {              // (every block's count is in: its ticket came behind its atomicAdd)
                const unsigned bad = __hip_atomic_exchange(h.bad_count, 0u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                *h.bad_flag = (long long)bad;
            }
            __threadfence_system();
            __hip_atomic_store(h.done_flag, (int64_t)h.done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The scaler (+ prior) as the epilogue of a sweep: what scaler_inverse_kernel does for 64 rows, for the 16 walkers
// of one workgroup.  X: the sweep's result in LDS, by rank of the first transform ([rank][16], lidx); rof: rank of
// every feature; scr: LDS scratch of scaler_epilogue_lds_bytes(D) bytes, 16-byte aligned.  Every thread of the
// workgroup calls it (it synchronises).
struct ScalerEpi {
    int on, have_prior;
    pmc_scaler_t s;
    pmc_prior_un_t pr;
    double* u_out; double* x_out; double* ldj_out; int32_t* finite_out; double* logp_out;
    pmc_handover_t h;                               // x' (column-major), finite mask, logp', row count and completion word
    long long* stamps;                              // measurement only (pmc_debug_set_epilogue_stamps): [block][8] of the 100 MHz clock
};

static inline size_t scaler_epilogue_lds_bytes(int D) {
    return (size_t)(2 * 16 * D + D * 17) * sizeof(double) + 16 * sizeof(int);
}

// the rows' part: log-determinant (numpy's pairwise sum of the Jacobian terms), finite mask, Prior.logpdf; then the
// column-major store of x and the completion word.  Every thread of the workgroup calls it behind a barrier that follows
// the last element.
__device__ __forceinline__ void scaler_epilogue_rows(const ScalerEpi& e, const double* Jt, const double* Pt, const double* Xt,
                                                     int* rowfin, int64_t row0, int64_t n, int D, int tid, int nthr) {
    const pmc_scaler_t& s = e.s;
    const pmc_handover_t& h = e.h;
    const int rows = (int)min((int64_t)16, n - row0);
    // Eight lanes per walker (nthr = 128: all 16 walkers at once; 64: two passes).  Lane i of a walker's group keeps numpy's
    // accumulator r_i of the pairwise sum (np_pairwise_leaf: a[i], a[i+8], ... in index order), the group combines them in
    // numpy's tree ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) and lane 0 adds the tail: the bits of np_pairwise_sum for D <= 128.
    // Prior.logpdf's sum is sequential by definition: lane 4 walks it, its terms loaded eight at a time ahead of the adds.
    const int n8 = D - (D % 8);
    for (int rb = 0; rb < 16; rb += nthr >> 3) {
        const int r = rb + (tid >> 3), i = tid & 7;
        const bool live = r < rows;
        const double* a = Jt + (size_t)r * D;
        double acc = 0.0;
        if (live && D >= 8) {
            acc = a[i];
            for (int k = i + 8; k < n8; k += 8) acc += a[k];
        }
        double lps = 0.0;
        if (live && e.have_prior && i == 4) {
            const double* P = Pt + (size_t)r * D;
            int j = 0;
            for (; j + 8 <= D; j += 8) {
                const double p0 = P[j], p1 = P[j + 1], p2 = P[j + 2], p3 = P[j + 3];
                const double p4 = P[j + 4], p5 = P[j + 5], p6 = P[j + 6], p7 = P[j + 7];
                lps += p0; lps += p1; lps += p2; lps += p3; lps += p4; lps += p5; lps += p6; lps += p7;
            }
            for (; j < D; ++j) lps += P[j];
        }
        // (every lane of the wavefront takes part in the exchanges; lane 0 of a group ends with numpy's operand order)
        acc = acc + __shfl_xor(acc, 1, 8);
        acc = acc + __shfl_xor(acc, 2, 8);
        acc = acc + __shfl_xor(acc, 4, 8);
        lps = __shfl(lps, 4, 8);
        if (live && i == 0) {
            double l;
            if (D < 8) {
                l = 0.0;
                for (int k = 0; k < D; ++k) l += a[k];
            } else {
                l = acc;
                for (int k = n8; k < D; ++k) l += a[k];
            }
            if (s.scale) l = s.sum_log_sigma + l;
            e.ldj_out[row0 + r] = l;
            const int fin = (rowfin[r] && isfinite(l)) ? 1 : 0;
            e.finite_out[row0 + r] = fin;
            if (h.finite_copy) h.finite_copy[row0 + r] = fin;
            bool clean = fin != 0;
            if (e.have_prior) {
                // Prior.logpdf of the finite rows (mcmc.py:105-107): the terms dimension after dimension
                const double lp = fin ? lps : -INFINITY;
                e.logp_out[row0 + r] = lp;
                if (h.logp_copy) h.logp_copy[row0 + r] = lp;
                clean = clean && isfinite(lp);
            }
            if (h.bad_count && !clean) atomicAdd(h.bad_count, 1u);            // (rows that the host's masks would drop: rare)
            if (h.fill_x) rowfin[r] = clean ? 1 : 0;                                // (from here on: "the row reaches the likelihood")
        }
    }
    if (h.fill_x) __syncthreads();
    if (e.stamps && tid == 0) e.stamps[blockIdx.x * 8 + 2] = wall_clock64();
    if (e.stamps && tid == 0) e.stamps[blockIdx.x * 8 + 3] = wall_clock64();
    if (h.x_colmajor) {
        // element el = j * rows + r; (j, r) step by nthr = dj * rows + dr without a division per element
        const int dj = nthr / rows, dr = nthr - dj * rows;
        int j = tid / rows, r = tid - j * rows;
        for (int el = tid; el < rows * D; el += nthr) {
            // (a row that does not reach the likelihood: the walker's current x in the host copy, see scaler_inverse_kernel)
            h.x_colmajor[(size_t)j * n + row0 + r] = (h.fill_x && !rowfin[r]) ? h.fill_x[(row0 + r) * D + j] : Xt[j * 17 + r];
            j += dj; r += dr;
            if (r >= rows) { r -= rows; ++j; }
        }
    }
    if (e.stamps && tid == 0) e.stamps[blockIdx.x * 8 + 4] = wall_clock64();
    handover_complete(h, e.stamps, tid);
}

template <class LIDX>
__device__ __forceinline__ void scaler_epilogue(const ScalerEpi& e, const float* X, const int* __restrict__ rof,
                                                double* scr, int64_t row0, int64_t n, int D, int tid, int nthr,
                                                LIDX lidx_of) {
    double* Jt = scr;                               // [16][D]
    double* Pt = Jt + 16 * D;                       // [16][D] prior terms
    double* Xt = Pt + 16 * D;                       // [D][17]
    int* rowfin = reinterpret_cast<int*>(Xt + D * 17);
    const int rows = (int)min((int64_t)16, n - row0);
    if (tid < 16) rowfin[tid] = 1;
    if (e.stamps && tid == 0) e.stamps[blockIdx.x * 8 + 0] = wall_clock64();
    // A thread keeps ONE feature: thread tid takes feature tid % D of the rows tid / D, + rpp, + 2 rpp, ... (D <= nthr: the
    // fused instances end at D = 64; the nthr % D threads left over rest).  Its feature's constants and rank are
    // requested here, in one batch ahead of the barrier, and stay in registers over its rows.
    const int rpp = nthr / D;
    const int r0 = tid / D, j = tid - r0 * D;
    const bool act = r0 < rpp;
    ScalerFeat f;
    int rk = 0;
    if (act) {
        scaler_feat_request(f, e.s, e.have_prior ? &e.pr : nullptr, j);
        rk = rof[j];
    }
    __syncthreads();
    if (act) {
        scaler_feat_finish(f, e.s, e.have_prior != 0);
        for (int r = r0; r < rows; r += rpp) {
            // the bijector, its Jacobian term, the boundary conditions, the prior factor: u / x to the device arrays, the
            // row tables Jt / Pt / Xt / rowfin in LDS
            double u = (double)X[lidx_of(rk, r)], x, J;
            scaler_element(e.s, f, u, x, J);
            const int64_t g = (row0 + r) * D + j;
            e.u_out[g] = u;
            e.x_out[g] = x;
            Xt[j * 17 + r] = x;
            Jt[r * D + j] = J;
            if (e.have_prior) Pt[r * D + j] = prior_term(f, x);
            if (!isfinite(x)) rowfin[r] = 0;
        }
    }
    __syncthreads();
    if (e.stamps && tid == 0) e.stamps[blockIdx.x * 8 + 1] = wall_clock64();
    scaler_epilogue_rows(e, Jt, Pt, Xt, rowfin, row0, n, D, tid, nthr);
}

#endif
