// Internal helpers shared by the .hip translation units.
#ifndef PMC_INTERNAL_H
#define PMC_INTERNAL_H

#include <hip/hip_runtime.h>
#include "../../include/pocomc_amd.h"

// A/B switches of measurement builds (make DEBUG_HOOKS=1): the product library never reads the environment.
#ifdef PMC_DEBUG_HOOKS
#include <stdlib.h>
static inline int pmc_env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
#else
#define pmc_env_int(name, dflt) (dflt)
#endif

int pmc_fail(const char* msg);
int pmc_fail_hip(hipError_t e, const char* what);
int pmc_check_launch(const char* what);

int pmc_launch_forward_wg(const pmc_maf_t* m, const float* x, float* z, float* ladj, float* log_prob, int64_t n,
                          hipStream_t stream, const int64_t* idx = nullptr);
// the spline instances of the bf16 forward kernel (maf_forward_bf16_nsf.hip), behind pmc_maf_forward_bf16's checks
int pmc_launch_forward_bf16_nsf(const pmc_maf_t* m, const uint16_t* image, int64_t per_t, const float* x, float* z, float* ladj,
                                float* log_prob, int64_t n, const int64_t* idx, hipStream_t stream);
// The flow inverse (inverse_plan.hip): ONE function decides which kernel instance a call launches; the launchers below
// launch what its plan names (pa: the fused proposal's arguments, propose_body.h; NULL for the plain inverse of z).
// fused: PMC_FUSED_NO -- the plan of pmc_maf_inverse(algo), or non-zero with that call's error message; PMC_FUSED_STEP --
// the fused proposal + inverse instance of the step, or sweep = PMC_SWEEP_NONE (return 0) when the stages are launched one
// by one; epilogue: the scaler runs inside it (want_epilogue: the caller's scaler / prior qualify; scaler_D: their width);
// PMC_FUSED_ANY -- the same for pmc_propose_inverse, which names the fused launch itself: AUTO's preference of the
// lane-per-walker sweep (the proposal as a launch of its own) does not apply.
enum { PMC_FUSED_NO = 0, PMC_FUSED_STEP = 1, PMC_FUSED_ANY = 2 };
struct ProposeArgs;
int pmc_plan_inverse(const pmc_maf_t* m, int64_t n, int algo, int fused, int want_epilogue, int scaler_D, pmc_inverse_plan_t* out);
int pmc_launch_inverse(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z, float* x,
                       float* ladj, int64_t n, hipStream_t stream);     // one switch over plan->sweep (maf_kernels.hip)
int pmc_launch_tri4(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z, float* x,
                    float* ladj, int64_t n, hipStream_t stream);
int pmc_launch_tri5(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z, float* x,
                    float* ladj, int64_t n, hipStream_t stream);
int pmc_launch_tri6(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z, float* x,
                    float* ladj, int64_t n, hipStream_t stream);
int pmc_launch_nsf2(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z, float* x,
                    float* ladj, int64_t n, hipStream_t stream);
int pmc_launch_inverse_tri_nsf(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z,
                               float* x, float* ladj, int64_t n, hipStream_t stream);
int pmc_launch_inverse_dpass_wg(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z,
                                float* x, float* ladj, int64_t n, hipStream_t stream);
int pmc_launch_inverse_wg_sweep(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z,
                                float* x, float* ladj, int64_t n, hipStream_t stream);
int pmc_launch_inverse_wg_nsf_sweep(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z,
                                    float* x, float* ladj, int64_t n, hipStream_t stream);
// The float32 trainer's chain-kernel instance (maf_train.hip): the launch's LDS bytes, or 0 where neither the full nor the
// lean buffer plan fits; *lean which one, *ksplit (may be NULL) the partial-tile staging, *full_bytes the full plan's size
size_t pmc_train_instance(const pmc_maf_t* m, int* lean, int* ksplit, size_t* full_bytes);
int pmc_launch_propose_mfma(int kind, const float* cur32, const double* cur64, const double* mu,
                            const double* inv_cov, const double* chol, double nu, double sigma, double cn_a,
                            const pmc_rng_t* rng, double* prop64, float* prop32, double* quad, double* quad_prop,
                            int64_t n, int32_t D, hipStream_t stream, const double* adapt = nullptr);
int pmc_launch_clip_adamw(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                          double beta1, double beta2, double eps, double wd, double max_norm, int64_t step,
                          float* sq_scratch, hipStream_t st);
// pmc_scaler_inverse_prior with the whole hand-over (pmc_handover_t), the step's row count and fill included: the number of
// rows that do not reach the likelihood into *bad_flag in front of the completion word, and the walkers' current x for
// those rows in the second copy of x'.  The kernel does what *h says: pmc_step_pre's decision (step.hip) is the only filter.
int pmc_scaler_inverse_prior_ex(const pmc_scaler_t* s, const pmc_prior_t* prior, const float* u_in, const double* u_in64,
                                double* u_out, double* x, double* logdetj, int32_t* finite, double* logp,
                                const pmc_handover_t* h, int64_t n, void* stream);
// pmc_propose with sigma / cn_a / mu taken from pmc_step_t.adapt_state (device) when adapt != NULL
int pmc_propose_adapt(int kind, const float* cur32, const double* cur64, const double* mu, const double* inv_cov,
                      const double* chol, double nu, double sigma, double cn_a, const pmc_rng_t* rng, double* prop64,
                      float* prop32, double* quad, double* quad_prop, int64_t n, int32_t D, void* stream,
                      const double* adapt);
// what the accept kernel's last block does with the sums (pmc_step_t.adapt_*)
struct pmc_adapt_args {
    double* state;
    int mode;
    double c_sigma, c_mu, cap, n_total;
    const double* other[7];     // sums of the other row ranges (pmc_step_t.adapt_other)
    int n_other;
};
// the device-likelihood step's accept (pmc_step_t.lik_x): logl' gated to -inf where fin is 0 or logp' is not finite; the
// last block writes calls_n - *bad_count to calls_out (pinned host) and zeroes *bad_count.  All NULL: no gate.
struct pmc_gate_args {
    const int32_t* fin;
    unsigned* bad_count;
    long long* calls_out;
    long long calls_n;
};
// the walkers' blobs (pmc_step_t.blob_cur / blob_prop) as rows of row_dwords 32-bit words: the accept launch copies the
// accepted rows' from prop to cur.  row_dwords 0: no blobs.
struct pmc_blob_args {
    uint32_t* cur;
    const uint32_t* prop;
    int row_dwords;
};
int pmc_accept_adapt(int kind, int preconditioned, pmc_state_t* cur, const pmc_proposal_t* prop, double beta, double nu,
                     const pmc_rng_t* rng, double* alpha_out, int32_t* accept_out, double* sums, double* sums_copy,
                     const pmc_done_t* done, void* workspace, int64_t n, int32_t D, void* stream,
                     const pmc_adapt_args* adapt, const pmc_gate_args* gate = nullptr,
                     const pmc_blob_args* blob = nullptr);
// what pmc_joint_blocks_pre refuses of its descriptor (joint_prior.hip), for the step's stage check as well: 0 with the
// blocks' total width in *DF and the table's in *Dr (either may be NULL), or pmc_fail's code with that entry's text
int pmc_joint_blocks_check(const pmc_joint_blocks_t* j, int* DF, int* Dr);

#endif
