// One factor of Prior.logpdf for every scipy.stats family the device knows (pmc_prior_t, include/pocomc_amd.h).  Used by
// prior_logpdf_kernel and scaler_inverse_kernel only: the epilogues of the fused sweeps keep the two-family prior_term of
// scaler_body.h, and a prior with a factor of another family takes the scaler launch of its own (pmc_step_pre).
//
// Each family is scipy's rv_continuous.logpdf: z = (x - loc) / scale, scipy's support test on z (closed, or open for
// lognorm / invgamma), then _logpdf(z) - log(scale), with _logpdf written the way scipy 1.x writes it -- the same
// operations in the same order, no FMA contraction -- so that the edges (+inf / -inf / -0.0, overflow of z * z, underflow
// of exp) fall where scipy's do.  Every constant that depends on the parameters only (gammaln, betaln, the truncated
// normal's log-mass, log(scale), ...) comes from the host in float64 (Prior.device_table).
#ifndef PMC_PRIOR_BODY_H
#define PMC_PRIOR_BODY_H

#include "scaler_body.h"

#pragma clang fp contract(off)

#define PMC_SQRT_2PI 2.5066282746310002            // np.sqrt(2 * np.pi)
#define PMC_NORM_PDF_LOGC 0.9189385332046727       // scipy.stats._continuous_distns._norm_pdf_logC

// scipy.special.xlogy / xlog1py: 0 where x == 0 and y is not NaN
__device__ __forceinline__ double pmc_xlogy(double x, double y) { return (x == 0.0 && !isnan(y)) ? 0.0 : x * log(y); }
__device__ __forceinline__ double pmc_xlog1py(double x, double y) { return (x == 0.0 && !isnan(y)) ? 0.0 : x * log1p(y); }

// scipy's _logpdf(z) of the extended families (3..14); NaN for a code the device does not know.  p0 .. p2: the family's
// rows of pmc_prior_t.par
__device__ __forceinline__ double prior_ext_logpdf(int fam, double z, double p0, double p1, double p2) {
    switch (fam) {
    case PMC_PRIOR_TRUNCNORM:        // _norm_logpdf(x) - _log_gauss_mass(a, b) on [a, b]
        if (!(z >= p0 && z <= p1)) return -INFINITY;
        return (-(z * z) / 2.0 - PMC_NORM_PDF_LOGC) - p2;
    case PMC_PRIOR_LOGUNIFORM:       // -log(x) - log(log(b) - log(a)) on [a, b]
        if (!(z >= p0 && z <= p1)) return -INFINITY;
        return -log(z) - p2;
    case PMC_PRIOR_LOGNORM: {        // _lognorm_logpdf on (0, inf): -log(x)**2 / (2 s**2) - log(s x sqrt(2 pi)), -inf at 0
        if (!(z > 0.0 && z < INFINITY)) return -INFINITY;
        const double lz = log(z);
        return -(lz * lz) / p1 - log(p0 * z * PMC_SQRT_2PI);
    }
    case PMC_PRIOR_HALFNORM:         // 0.5 log(2/pi) - x*x/2 on [0, inf]
        if (!(z >= 0.0)) return -INFINITY;
        return p2 - z * z / 2.0;
    case PMC_PRIOR_EXPON:            // -x on [0, inf]
        if (!(z >= 0.0)) return -INFINITY;
        return -z;
    case PMC_PRIOR_GAMMA:            // xlogy(a-1, x) - x - gammaln(a) on [0, inf]
        if (!(z >= 0.0)) return -INFINITY;
        return pmc_xlogy(p0, z) - z - p2;
    case PMC_PRIOR_INVGAMMA:         // -(a+1) log(x) - gammaln(a) - 1/x on (0, inf)
        if (!(z > 0.0 && z < INFINITY)) return -INFINITY;
        return -p0 * log(z) - p2 - 1.0 / z;
    case PMC_PRIOR_BETA: {           // xlog1py(b-1, -x) + xlogy(a-1, x) - betaln(a, b) on [0, 1]
        if (!(z >= 0.0 && z <= 1.0)) return -INFINITY;
        double l = pmc_xlog1py(p1, -z) + pmc_xlogy(p0, z);
        l -= p2;
        return l;
    }
    case PMC_PRIOR_CAUCHY: {         // -log(pi) - log1p(|x|**2), or -log(pi) - (2 log|x| + log1p((1/|x|)**2)) for |x| >= 1
        const double a = fabs(z);
        if (a < 1.0) return -p2 - log1p(a * a);
        const double r = 1.0 / a;
        return -p2 - (2.0 * log(a) + log1p(r * r));
    }
    case PMC_PRIOR_HALFCAUCHY:       // log(2/pi) - log1p(x*x) on [0, inf]
        if (!(z >= 0.0)) return -INFINITY;
        return p2 - log1p(z * z);
    case PMC_PRIOR_LAPLACE:          // rv_continuous._logpdf: log(_pdf(x)) = log(0.5 exp(-|x|))
        return log(0.5 * exp(-fabs(z)));
    case PMC_PRIOR_T:                // log(poch(df/2, 1/2)) - (log(df) + log(pi))/2 - (df+1)/2 log1p(x*x/df); df = inf: norm
        if (isinf(p0)) return -(z * z) / 2.0 - PMC_NORM_PDF_LOGC;
        return p2 - p1 * log1p(z * z / p0);
    default:
        return NAN;
    }
}

// one factor of Prior.logpdf, any family: uniform / normal exactly as prior_term (the same bits as the fused epilogues);
// the others need pr.par (pmc_prior_logpdf and pmc_scaler_inverse_prior refuse a descriptor with n_extended > 0 without it)
__device__ __forceinline__ double prior_term_any(const pmc_prior_t& pr, int j, double xv) {
    const int fam = pr.family[j];
    if (fam == PMC_PRIOR_UNIFORM || fam == PMC_PRIOR_NORM) return prior_term(pr, j, xv);
    if (!pr.par) return NAN;
    const int D = pr.D;
    const double z = (xv - pr.loc[j]) / pr.scale[j];
    return prior_ext_logpdf(fam, z, pr.par[j], pr.par[D + j], pr.par[2 * D + j]) - pr.par[3 * D + j];
}

#endif
