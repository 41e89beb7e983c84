// Composite entry points of one MCMC step (pocomc/mcmc.py:74-149): everything the device does
// before and after the host's prior / likelihood call, enqueued by ONE C call each, so that the
// host-side driver spends its time in the user's black boxes instead of in dispatch overhead.
//
//   pmc_step_pre :  [H2D mu] -> propose -> flow inverse (one launch for the affine flows) -> scaler inverse [+ prior] -> D2H x', finite
//                   [-> the flow / joint prior's three launches on p_x, pmc_step_ext_t.prior_stage; the blocks form's B + 2,
//                       pmc_step_ext2_t.blocks_stage]
//   pmc_step_post:  H2D logl', logp' -> accept + reductions -> D2H sums
//
// With a likelihood on the device (pmc_step_t.lik_x) x' goes to lik_x instead of the host, the caller's likelihood fills
// p_logl on the same stream, and the accept gates logl' itself: no copy of x' or logl' in either direction.
// A prior that is a GPU callable too (pmc_step_t.prior_rows) sits between the two: pmc_step_prior_rows takes its values.
//
// Pure sequencing of the single-purpose entry points (same kernels, same stream order); host
// buffers must be pinned for the copies to be asynchronous.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <time.h>
#include "pmc_internal.h"
#include "propose_body.h"
#include "blob_move.h"
#include "flow_prior_body.h"

#ifdef PMC_DEBUG_HOOKS                               // measurement builds only (make DEBUG_HOOKS=1): not in the product library
static long long* g_epilogue_stamps = nullptr;       // pmc_debug_set_epilogue_stamps
static int64_t g_epilogue_stamps_n = 0;
static bool g_stage_per_lane = false;                // pmc_debug_set_stage_per_lane
#endif

// the variates of step rng->step + 1 into the other parity's buffers (throughput mode, see pmc_step_t.rng_normal)
static bool step_prefills(const pmc_step_t* s, const pmc_rng_t* rng) {
    return s->rng_ready && s->rng_normal[0] && s->rng_normal[1] && s->rng_uniform[0] && s->rng_uniform[1] &&
           (s->kind != PMC_KIND_TPCN || (s->rng_gamma[0] && s->rng_gamma[1])) && !rng->normal && !rng->gamma && !rng->uniform;
}

extern "C" int pmc_step_fill_next(const pmc_step_t* s, const pmc_rng_t* rng, double nu, void* stream) {
    if (!s || !rng) return pmc_fail("pmc_step_fill_next: null argument");
    if (!step_prefills(s, rng)) return 0;
    const int rb = (int)(rng->step & 1);
    const double gshape = (s->kind == PMC_KIND_TPCN) ? 0.5 * ((double)s->D + nu) : 0.0;      // mcmc.py:80
    pmc_rng_t nx = *rng;
    nx.step = rng->step + 1;
    int rcf = pmc_rng_fill(&nx, gshape, s->rng_normal[rb ^ 1], s->rng_gamma[rb ^ 1], s->rng_uniform[rb ^ 1], s->n, s->D, stream);
    if (rcf) return rcf;
    *s->rng_ready = (int64_t)nx.step;
    return 0;
}

// the fields behind a pmc_step_t that is the head of a pmc_step_ext_t (step.ext says so; nothing behind it is read otherwise)
// (pmc_step_ext2_t begins as pmc_step_ext_t does: prior_stage sits at one offset in both)
static const pmc_prior_stage_t* step_stage(const pmc_step_t* s) {
    return (s->ext == PMC_STEP_EXT || s->ext == PMC_STEP_EXT2) ? reinterpret_cast<const pmc_step_ext_t*>(s)->prior_stage : nullptr;
}
static const pmc_prior_blocks_stage_t* step_blocks_stage(const pmc_step_t* s) {
    return s->ext == PMC_STEP_EXT2 ? reinterpret_cast<const pmc_step_ext2_t*>(s)->blocks_stage : nullptr;
}
// a stage of either kind (pmc_step_ext_t.prior_stage, pmc_step_ext2_t.blocks_stage)
static bool step_has_stage(const pmc_step_t* s) { return step_stage(s) || step_blocks_stage(s); }
// a copy the caller may change: the head, and the fields behind it where there are any
static pmc_step_ext2_t step_copy(const pmc_step_t* s) {
    pmc_step_ext2_t c{};
    c.step = *s;
    c.prior_stage = step_stage(s);
    c.blocks_stage = step_blocks_stage(s);
    return c;
}

// host_direct: the kernels read mu from / write x', finite, logp' to pinned host memory themselves
static bool step_direct(const pmc_step_t* s) { return s->host_direct && !s->p_xT; }

// the pre-step's device likelihood: x' stays on the device only behind a prior that is evaluated there too
static bool step_devlik(const pmc_step_t* s) { return s->lik_x && (s->prior || s->prior_rows); }

// where x' goes and where logl' / logp' come from (PMC_HANDOVER_*); devlik: the caller's, see pmc_step_post
static int step_mode(const pmc_step_t* s, bool devlik) {
    return devlik ? PMC_HANDOVER_DEVLIK : step_direct(s) ? PMC_HANDOVER_DIRECT : PMC_HANDOVER_COPIES;
}

// THE decision of the pre-step of step number `step` about x', the finite mask, logp', the row count and the completion
// word (pmc_step_handover has the outputs); epilogue: the plan's fused sweep runs the scaler, else a launch of its own.
//   device likelihood with a device prior: x' (rejected rows filled) into lik_x, the count into clean_count; nothing goes
//   to the host and no completion word follows (the likelihood is the next operation on the stream).  A prior that is the
//   caller's GPU callable (prior_rows): the same hand-over with the finite mask as the only gate -- pmc_step_prior_rows
//   closes the prior's behind the callable.
//   host_direct: everything into pinned host memory, the completion word behind it where the caller gave one; the rows
//   that do not reach the likelihood are counted into *h_clean in front of the word (and their host rows filled when asked).
// One asymmetry, kept as it is: the fused epilogue counts whenever it has the word, h_clean and clean_count -- without a
// device prior too (the rows whose x' is not finite), and without a host x' -- while the launch of its own counts only
// when it hands x' over and evaluates the prior.  (The epilogues evaluate uniform / normal factors only: a prior with a
// factor of another family keeps the launch of its own, which counts, fills and hands over x' the same way.)
static void step_handover(const pmc_step_t* s, int64_t step, bool epilogue, pmc_handover_t* h, int32_t* mode,
                          int32_t* clean_unknown) {
    const bool devlik = step_devlik(s);
    *mode = step_mode(s, devlik);
    const bool host = *mode == PMC_HANDOVER_DIRECT;
    *h = pmc_handover_t{};
    h->x_colmajor = devlik ? s->lik_x : step_direct(s) ? s->h_x : s->p_xT;
    if (host) {
        h->finite_copy = s->h_fin;
        if (s->prior) h->logp_copy = s->h_logp_out;
    }
    const bool done = host && s->h_done && s->done_ticket;
    if (done) { h->done_ticket = s->done_ticket; h->done_flag = s->h_done; h->done_value = step + 1; }
    const bool word = done && s->h_clean && s->clean_count;             // the count has somewhere to go
    if (word && (epilogue || (h->x_colmajor && s->prior))) {
        h->bad_count = s->clean_count;
        h->bad_flag = s->h_clean;
        if (s->fill_rejected && h->x_colmajor) h->fill_x = s->cur.x;
    }
    if (devlik) { h->bad_count = s->clean_count; h->bad_flag = nullptr; h->fill_x = s->cur.x; }
    *clean_unknown = s->h_clean && !(word && h->x_colmajor && (epilogue || s->prior));
}

extern "C" int pmc_step_handover(const pmc_step_t* s, int64_t step, int32_t epilogue, pmc_handover_t* out, int32_t* mode,
                                 int32_t* clean_unknown) {
    if (!s || !out || !mode || !clean_unknown) return pmc_fail("pmc_step_handover: null argument");
    step_handover(s, step, epilogue != 0, out, mode, clean_unknown);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// The flow / joint prior of a host likelihood on the step's stream (pmc_step_ext_t.prior_stage, pmc_step_prior_stage).
//
// The closing kernel: one thread per walker.  logp' as the priors' own post kernels join it (flow_prior_body.h), -inf
// where x' is not finite (mcmc.py:105-107).  The rows with a finite x' and no finite logp' -- the host hands them to the
// likelihood, the reference does not (mcmc.py:108-109) -- are counted: a ballot per wavefront, one atomic per block on
// count[0], whose high half counts the blocks that have arrived and whose low half the rows.  The block that finds every
// other one arrived stores the total to h_count[launch & 1] (count[1]: the launches so far) and leaves count[0] at zero
// for the next launch; nothing else in the kernel depends on another block.  The launch ends, that store included,
// before the next launch on the stream -- the accept -- starts.
template <bool JOINT>
__global__ __launch_bounds__(256) void prior_stage_close_kernel(const float* __restrict__ lp32, const double* __restrict__ ldj,
                                                                const double* __restrict__ rest_logp,
                                                                const int32_t* __restrict__ inside,
                                                                const int32_t* __restrict__ fin, double* __restrict__ logp,
                                                                unsigned long long* __restrict__ count,
                                                                long long* __restrict__ h_count, int64_t n) {
    __shared__ unsigned wave_bad[4];
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * 256 + tid;
    bool bad = false;
    if (r < n) {
        double v = -INFINITY;
        if (fin[r]) {
            v = JOINT ? joint_prior_join(lp32[r], ldj[r], rest_logp[r], inside[r]) : flow_prior_join(lp32[r], ldj[r], inside[r]);
            bad = !isfinite(v);
        }
        logp[r] = v;
    }
    const unsigned nb = (unsigned)__popcll(__ballot(bad));
    if ((tid & 63) == 0) wave_bad[tid >> 6] = nb;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long mine = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
        const unsigned long long old = __hip_atomic_fetch_add(count, (1ull << 32) | mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(old >> 32) == gridDim.x - 1) {
            const unsigned long long launch = count[1];
            __hip_atomic_store(h_count + (launch & 1), (long long)((old & 0xffffffffull) + mine), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
            count[1] = launch + 1;
            __hip_atomic_store(count, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// The blocks form of the joint prior (pmc_step_ext2_t.blocks_stage): the closing kernel of the stage above with the join
// over several blocks (joint_blocks_join: lp32 / ldj [n_blocks][n], rest_logp NULL without a table) -- the same count
// protocol, word for word.
__global__ __launch_bounds__(256) void prior_blocks_stage_close_kernel(int n_blocks, const float* __restrict__ lp32,
                                                                       const double* __restrict__ ldj,
                                                                       const double* __restrict__ rest_logp,
                                                                       const int32_t* __restrict__ inside,
                                                                       const int32_t* __restrict__ fin, double* __restrict__ logp,
                                                                       unsigned long long* __restrict__ count,
                                                                       long long* __restrict__ h_count, int64_t n) {
    __shared__ unsigned wave_bad[4];
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * 256 + tid;
    bool bad = false;
    if (r < n) {
        double v = -INFINITY;
        if (fin[r]) {
            v = joint_blocks_join(n_blocks, lp32, ldj, rest_logp, inside[r], n, r);
            bad = !isfinite(v);
        }
        logp[r] = v;
    }
    const unsigned nb = (unsigned)__popcll(__ballot(bad));
    if ((tid & 63) == 0) wave_bad[tid >> 6] = nb;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long mine = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
        const unsigned long long old = __hip_atomic_fetch_add(count, (1ull << 32) | mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((unsigned)(old >> 32) == gridDim.x - 1) {
            const unsigned long long launch = count[1];
            __hip_atomic_store(h_count + (launch & 1), (long long)((old & 0xffffffffull) + mine), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
            count[1] = launch + 1;
            __hip_atomic_store(count, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// what the step refuses of a stage of either kind (the texts of prior_stage_check below)
static int stage_step_check(const pmc_step_t* s) {
    if (s->prior) return pmc_fail("pmc_step_prior_stage: the step has a device prior table as well (prior): one of the two");
    if (s->prior_rows) return pmc_fail("pmc_step_prior_stage: the step has a prior that is a GPU callable as well (prior_rows): one of the two");
    if (s->lik_x) return pmc_fail("pmc_step_prior_stage: the stage is for a host likelihood (lik_x is set: call the prior on lik_x instead)");
    return 0;
}

// the blocks branch of prior_stage_check: the same order -- the step, the stage's pointers, the rows, the widths
static int blocks_stage_check(const pmc_step_t* s, const pmc_prior_blocks_stage_t* g) {
    if (int e = stage_step_check(s)) return e;
    const int B = g->blocks.n_blocks;
    if (B < 1 || B > PMC_JOINT_BLOCKS_MAX) return pmc_fail("pmc_joint_blocks_pre: n_blocks must lie in 1 .. 8");
    for (int b = 0; b < B; ++b)
        if (!g->blocks.scaler[b] || !g->maf[b]) return pmc_fail("pmc_step_prior_stage: every block needs its scaler and its flow");
    if (!g->u32 || !g->z || !g->lp32 || !g->ldj || !g->inside) return pmc_fail("pmc_step_prior_stage: null workspace (u32, z, lp32, ldj, inside)");
    if (!g->count || !g->h_count) return pmc_fail("pmc_step_prior_stage: needs the device counter and the pinned host words");
    if (g->blocks.rest && !g->rest_logp) return pmc_fail("pmc_step_prior_stage: null workspace (rest_logp)");
    for (int b = 0; b < B; ++b)
        if (g->image16[b] && g->image_per_transform[b] < 1) return pmc_fail("pmc_step_prior_stage: a bf16 image needs image_per_transform");
    if (s->n < 1) return pmc_fail("pmc_step_prior_stage: n < 1");
    if (s->n > 0x7fffffffLL) return pmc_fail("pmc_step_prior_stage: too many rows for one count");
    if (!s->p_x || !s->p_fin || !s->p_logp) return pmc_fail("pmc_step_prior_stage: needs p_x, p_fin and p_logp");
    int DF = 0, Dr = 0;
    if (int e = pmc_joint_blocks_check(&g->blocks, &DF, &Dr)) return e;     // (what pmc_joint_blocks_pre refuses, in its words)
    if (DF + Dr != s->D || (g->blocks.D != 0 && g->blocks.D != s->D))
        return pmc_fail("pmc_step_prior_stage: the prior's width is not the step's D");
    for (int b = 0; b < B; ++b)
        if (g->maf[b]->D != g->blocks.scaler[b]->D) return pmc_fail("pmc_step_prior_stage: the flow's width is not the scaler's");
    return 0;
}

// the B + 2 launches (the struct has passed blocks_stage_check)
static int blocks_stage_enqueue(const pmc_step_t* s, const pmc_prior_blocks_stage_t* g, void* stream) {
    const int64_t n = s->n;
    const int B = g->blocks.n_blocks;
    int rc = pmc_joint_blocks_pre(&g->blocks, s->p_x, s->D, 1, n, g->u32, g->ldj, g->rest_logp, g->inside, stream);
    if (rc) return rc;
    int64_t off = 0;
    for (int b = 0; b < B; ++b) {                   // block b's piece of u32 and its row of lp32; one z for all: nobody reads it
        float* u = g->u32 + n * off;
        float* lp = g->lp32 + (int64_t)b * n;
        rc = g->image16[b] ? pmc_maf_forward_bf16(g->maf[b], g->image16[b], g->image_per_transform[b], u, g->z, nullptr, lp, n, nullptr, stream)
                           : pmc_maf_forward(g->maf[b], u, g->z, nullptr, lp, n, stream);
        if (rc) return rc;
        off += g->blocks.scaler[b]->D;
    }
    hipLaunchKernelGGL(prior_blocks_stage_close_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B,
                       g->lp32, g->ldj, g->blocks.rest ? g->rest_logp : (const double*)nullptr, g->inside, s->p_fin, s->p_logp,
                       g->count, (long long*)g->h_count, n);
    return pmc_check_launch("prior_blocks_stage_close_kernel");
}

// what pmc_step_prior_stage refuses, before any launch (host logic: follows s->prior_stage and its scaler / rest only)
static int prior_stage_check(const pmc_step_t* s) {
    if (!s) return pmc_fail("pmc_step_prior_stage: null argument");
    const pmc_prior_stage_t* g = step_stage(s);
    if (const pmc_prior_blocks_stage_t* gb = step_blocks_stage(s)) {
        if (g) return pmc_fail("pmc_step_prior_stage: prior_stage and blocks_stage are both set: one of the two");
        return blocks_stage_check(s, gb);
    }
    if (!g) return pmc_fail("pmc_step_prior_stage: the step has no prior_stage");
    if (s->prior) return pmc_fail("pmc_step_prior_stage: the step has a device prior table as well (prior): one of the two");
    if (s->prior_rows) return pmc_fail("pmc_step_prior_stage: the step has a prior that is a GPU callable as well (prior_rows): one of the two");
    if (s->lik_x) return pmc_fail("pmc_step_prior_stage: the stage is for a host likelihood (lik_x is set: call the prior on lik_x instead)");
    if (!g->scaler || !g->maf) return pmc_fail("pmc_step_prior_stage: needs the flow block's scaler and the flow");
    if (!g->u32 || !g->z || !g->lp32 || !g->ldj || !g->inside) return pmc_fail("pmc_step_prior_stage: null workspace (u32, z, lp32, ldj, inside)");
    if (!g->count || !g->h_count) return pmc_fail("pmc_step_prior_stage: needs the device counter and the pinned host words");
    const bool joint = g->flow_cols || g->rest || g->rest_cols;
    if (joint && !(g->flow_cols && g->rest && g->rest_cols)) return pmc_fail("pmc_step_prior_stage: a joint prior needs flow_cols, rest and rest_cols");
    if (joint && !g->rest_logp) return pmc_fail("pmc_step_prior_stage: null workspace (rest_logp)");
    if (g->image16 && g->image_per_transform < 1) return pmc_fail("pmc_step_prior_stage: a bf16 image needs image_per_transform");
    if (s->n < 1) return pmc_fail("pmc_step_prior_stage: n < 1");
    if (s->n > 0x7fffffffLL) return pmc_fail("pmc_step_prior_stage: too many rows for one count");
    if (!s->p_x || !s->p_fin || !s->p_logp) return pmc_fail("pmc_step_prior_stage: needs p_x, p_fin and p_logp");
    // the widths the two *_pre entries refuse, in their words
    const int64_t Df = g->scaler->D, Dr = joint ? g->rest->D : 0;
    if (!joint && Df < 1) return pmc_fail("pmc_flow_prior_pre: bad descriptor");
    if (!joint && Df > FP_MAX_D) return pmc_fail("pmc_flow_prior_pre: n_dim too large (D <= 157)");
    if (joint && Df < 2) return pmc_fail("pmc_joint_prior_pre: the flow block needs at least 2 columns (Df >= 2)");
    if (joint && Dr < 1) return pmc_fail("pmc_joint_prior_pre: the rest needs at least 1 factor (Dr >= 1)");
    if (joint && Df + Dr > FP_MAX_D) return pmc_fail("pmc_joint_prior_pre: n_dim too large (Df + Dr <= 157)");
    if (Df + Dr != s->D) return pmc_fail("pmc_step_prior_stage: the prior's width is not the step's D");
    if (g->maf->D != Df) return pmc_fail("pmc_step_prior_stage: the flow's width is not the scaler's");
    return 0;
}

// the three launches (the struct has passed prior_stage_check)
static int prior_stage_enqueue(const pmc_step_t* s, void* stream) {
    if (const pmc_prior_blocks_stage_t* gb = step_blocks_stage(s)) return blocks_stage_enqueue(s, gb, stream);
    const pmc_prior_stage_t* g = step_stage(s);
    const int64_t n = s->n;
    const bool joint = g->flow_cols != nullptr;
    int rc = joint ? pmc_joint_prior_pre(g->scaler, g->flow_cols, g->rest, g->rest_cols, s->p_x, s->D, 1, n, g->u32, g->ldj,
                                         g->rest_logp, g->inside, stream)
                   : pmc_flow_prior_pre(g->scaler, s->p_x, s->D, 1, n, g->u32, g->ldj, g->inside, stream);
    if (rc) return rc;
    rc = g->image16 ? pmc_maf_forward_bf16(g->maf, g->image16, g->image_per_transform, g->u32, g->z, nullptr, g->lp32, n, nullptr, stream)
                    : pmc_maf_forward(g->maf, g->u32, g->z, nullptr, g->lp32, n, stream);
    if (rc) return rc;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (joint)
        hipLaunchKernelGGL(prior_stage_close_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, g->lp32, g->ldj, g->rest_logp,
                           g->inside, s->p_fin, s->p_logp, g->count, (long long*)g->h_count, n);
    else
        hipLaunchKernelGGL(prior_stage_close_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, g->lp32, g->ldj,
                           (const double*)nullptr, g->inside, s->p_fin, s->p_logp, g->count, (long long*)g->h_count, n);
    return pmc_check_launch("prior_stage_close_kernel");
}

extern "C" int pmc_step_prior_stage(const pmc_step_t* s, void* stream) {
    if (int e = prior_stage_check(s)) return e;
    return prior_stage_enqueue(s, stream);
}

// fill_next = false: the caller enqueues pmc_step_fill_next itself, behind whatever the host waits for first (the pipeline:
// behind the last lane's pre-step)
static int step_pre(const pmc_step_t* s, const pmc_rng_t* rng, double nu, double sigma, double cn_a, void* stream,
                    bool fill_next) {
    if (!s || !rng) return pmc_fail("pmc_step_pre: null argument");
    if (step_has_stage(s)) { if (int e = prior_stage_check(s)) return e; }      // (before the pre-step's own launches)
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = s->n;
    const int32_t D = s->D;
    const bool tpcn = (s->kind == PMC_KIND_TPCN);
    // throughput mode: this step's Philox variates were drawn ahead of time (see pmc_step_t.rng_normal)
    pmc_rng_t rr = *rng;
    const bool prefill = step_prefills(s, rng);
    const pmc_rng_t* rng_in = rng;
    const int rb = (int)(rng->step & 1);
    const double gshape = tpcn ? 0.5 * ((double)D + nu) : 0.0;             // mcmc.py:80
    if (prefill) {
        if (*s->rng_ready != (int64_t)rng->step) {                       // first step of a run
            int rcf = pmc_rng_fill(rng, gshape, s->rng_normal[rb], s->rng_gamma[rb], s->rng_uniform[rb], n, D, stream);
            if (rcf) return rcf;
        }
        rr.normal = s->rng_normal[rb];
        rr.gamma = tpcn ? s->rng_gamma[rb] : nullptr;
        rng = &rr;
    }
    // what follows the last kernel whose results the host waits for
    auto finish = [&]() -> int {
        if (s->ev_pre_done) (void)hipEventRecord((hipEvent_t)s->ev_pre_done, st);
        // the flow / joint prior of a host likelihood: behind everything the host waits for, while it evaluates the
        // likelihood; in front of the next step's variates, which nothing of this step needs (fill_next = false: the
        // caller places the stage as it places the fill)
        if (step_has_stage(s) && fill_next) { if (int e = prior_stage_enqueue(s, stream)) return e; }
        if (prefill && fill_next) return pmc_step_fill_next(s, rng_in, nu, stream);
        return 0;
    };
    const double* mu = s->mu;
    // adaptation on the device: sigma, cn_a and mu come from adapt_state (pmc_step_post keeps it up to date)
    const double* adapt = (s->adapt_state && s->adapt_mode) ? s->adapt_state : nullptr;
    if (!adapt && tpcn && s->h_mu) {
        if (step_direct(s)) mu = s->h_mu;
        else if (hipMemcpyAsync((void*)s->mu, s->h_mu, (size_t)D * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
            return pmc_fail("pmc_step_pre: H2D mu");
    }
    int rc;
    // scaler inverse and (when it runs on the device) Prior.logpdf: one launch, or the epilogue of the fused sweep
    const pmc_prior_t* pr = s->prior;
    double* lp = pr ? s->p_logp : nullptr;
    if (step_devlik(s) && !s->clean_count) return pmc_fail("pmc_step_pre: a device likelihood needs clean_count");
    // proposal + flow inverse (+ scaler) in one launch where the plan has such an instance (inverse_plan.hip: affine flows of
    // D <= 64 and < 16 hidden tiles, spline flows of D <= 64); no_fuse & 1 keeps the stages apart, no_fuse & 2 the scaler
    const bool want_epi = s->preconditioned && !(s->no_fuse & 3) && s->scaler && s->scaler->low && s->scaler->high &&
                          s->scaler->kind && s->scaler->log_width && (!s->scaler->scale || (s->scaler->mu && s->scaler->sigma)) &&
                          (!pr || (pr->family && pr->loc && pr->scale && pr->D == D && pr->n_extended == 0));
    pmc_inverse_plan_t plan{};
    if (s->preconditioned && !(s->no_fuse & 1)) {
        rc = pmc_plan_inverse(s->maf, n, s->inverse_algo, PMC_FUSED_STEP, want_epi, want_epi ? s->scaler->D : 0, &plan);
        if (rc) return rc;
    }
    pmc_handover_t hand;
    int32_t mode, clean_unknown;
    step_handover(s, (int64_t)rng->step, plan.epilogue != 0, &hand, &mode, &clean_unknown);
    // (this launch sequence does not count.  No kernel writes the word then, so the store may stand in front of the launches:
    //  a pre-step that fails in one of them leaves "not known" behind, not the count of an earlier step)
    if (clean_unknown) *s->h_clean = -1;
    if (plan.sweep != PMC_SWEEP_NONE) {
        ProposeArgs pa{s->kind, s->cur.theta32, mu, s->inv_cov, s->chol, nu, sigma, cn_a, *rng, s->p_theta64,
                       tpcn ? s->quad : nullptr, tpcn ? s->p_quad : nullptr, adapt};
        if (plan.epilogue) {
            ScalerEpi& epi = pa.epi;
            epi.on = 1;
            epi.s = *s->scaler;
            epi.have_prior = pr ? 1 : 0;
            if (pr) epi.pr = pmc_prior_un_t{pr->family, pr->loc, pr->scale, pr->D, pr->reserved};
            epi.u_out = s->p_u; epi.x_out = s->p_x; epi.ldj_out = s->p_logdetj; epi.finite_out = s->p_fin; epi.logp_out = lp;
            epi.h = hand;
#ifdef PMC_DEBUG_HOOKS
            epi.stamps = (n == g_epilogue_stamps_n) ? g_epilogue_stamps : nullptr;
#endif
        }
        if (s->ev_inv0) (void)hipEventRecord((hipEvent_t)s->ev_inv0, st);
        rc = pmc_launch_inverse(&plan, &pa, s->maf, nullptr, s->p_u32, s->p_ldjf, n, st);
        if (rc) return rc;
        if (s->ev_inv1) (void)hipEventRecord((hipEvent_t)s->ev_inv1, st);
    } else {
        rc = pmc_propose_adapt(s->kind, s->preconditioned ? s->cur.theta32 : nullptr,
                               s->preconditioned ? nullptr : s->cur.u, mu, s->inv_cov, s->chol, nu, sigma, cn_a, rng,
                               s->p_theta64, s->preconditioned ? s->p_theta32 : nullptr, tpcn ? s->quad : nullptr,
                               tpcn ? s->p_quad : nullptr, n, D, stream, adapt);
        if (rc) return rc;
        if (s->preconditioned) {
            if (s->ev_inv0) (void)hipEventRecord((hipEvent_t)s->ev_inv0, st);
            rc = pmc_maf_inverse(s->maf, s->p_theta32, s->p_u32, s->p_ldjf, n, s->inverse_algo, stream);
            if (s->ev_inv1) (void)hipEventRecord((hipEvent_t)s->ev_inv1, st);
            if (rc) return rc;
        }
    }
    if (!plan.epilogue) {                             // the scaler launch of its own
        rc = pmc_scaler_inverse_prior_ex(s->scaler, pr, s->preconditioned ? s->p_u32 : nullptr,
                                         s->preconditioned ? nullptr : s->p_theta64, s->p_u, s->p_x, s->p_logdetj, s->p_fin,
                                         lp, &hand, n, stream);
        if (rc) return rc;
    }
    if (mode != PMC_HANDOVER_COPIES) return finish();
    if (pr) {
        if (hipMemcpyAsync(s->h_logp_out, s->p_logp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess)
            return pmc_fail("pmc_step_pre: D2H logp");
    }
    const double* xsrc = s->p_xT ? s->p_xT : s->p_x;
    if (hipMemcpyAsync(s->h_x, xsrc, (size_t)n * D * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(s->h_fin, s->p_fin, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess)
        return pmc_fail("pmc_step_pre: D2H");
    return finish();
}

extern "C" int pmc_step_pre(const pmc_step_t* s, const pmc_rng_t* rng, double nu, double sigma, double cn_a,
                            void* stream) {
    return step_pre(s, rng, nu, sigma, cn_a, stream, true);
}

extern "C" int pmc_step_pre_deferred(const pmc_step_t* s, const pmc_rng_t* rng, double nu, double sigma, double cn_a,
                                     void* stream) {
    return step_pre(s, rng, nu, sigma, cn_a, stream, false);
}

// A device likelihood's input behind a host prior (pmc_step_lik_rows): one thread per walker, x' or the current x of its
// row into the column-major lik_x (coalesced along the walkers)
__global__ __launch_bounds__(256) void lik_rows_kernel(const double* __restrict__ x_prop, const double* __restrict__ x_cur,
                                                       const int32_t* __restrict__ fin, const double* __restrict__ logp,
                                                       double* __restrict__ lik_x, unsigned* __restrict__ bad_count,
                                                       int64_t n, int D) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const bool reach = fin[r] && isfinite(logp[r]);                 // mcmc.py:108-109
    const double* src = (reach ? x_prop : x_cur) + r * D;
    for (int j = 0; j < D; ++j) lik_x[(size_t)j * n + r] = src[j];
    if (!reach) atomicAdd(bad_count, 1u);
}

extern "C" int pmc_step_lik_rows(const pmc_step_t* s, void* stream) {
    if (!s || !s->lik_x || !s->clean_count || !s->p_x || !s->cur.x || !s->p_fin || !s->p_logp || !s->h_logp || s->D < 1)
        return pmc_fail("pmc_step_lik_rows: needs lik_x, clean_count, p_x, cur.x, p_fin, p_logp and h_logp");
    if (s->prior) return pmc_fail("pmc_step_lik_rows: with a device prior pmc_step_pre fills lik_x itself");
    const int64_t n = s->n;
    if (n <= 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(s->p_logp, s->h_logp, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
        return pmc_fail("pmc_step_lik_rows: H2D logp");
    hipLaunchKernelGGL(lik_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->p_x, s->cur.x, s->p_fin,
                       s->p_logp, s->lik_x, s->clean_count, n, (int)s->D);
    return pmc_check_launch("lik_rows_kernel");
}

// The values of a prior that is a GPU callable (pmc_step_prior_rows): one thread per walker; logp' into p_logp, and the row
// of a finite x' whose logp' is not finite back to the walker's current x in the column-major lik_x (coalesced along the
// walkers).  The rows whose x' is not finite were filled and counted by the pre-step.
__global__ __launch_bounds__(256) void prior_rows_kernel(const void* __restrict__ logp_in, int is_f32,
                                                         const double* __restrict__ x_cur, const int32_t* __restrict__ fin,
                                                         double* __restrict__ logp, double* __restrict__ lik_x,
                                                         unsigned* __restrict__ bad_count, int64_t n, int D) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    if (!fin[r]) { logp[r] = -INFINITY; return; }                   // mcmc.py:105-107
    const double v = is_f32 ? (double)static_cast<const float*>(logp_in)[r] : static_cast<const double*>(logp_in)[r];
    logp[r] = v;                                                    // (a NaN as it came: the accept's gate and NaN -> 0 rule see it)
    if (isfinite(v)) return;                                        // mcmc.py:108-109
    const double* src = x_cur + r * D;
    for (int j = 0; j < D; ++j) lik_x[(size_t)j * n + r] = src[j];
    atomicAdd(bad_count, 1u);
}

extern "C" int pmc_step_prior_rows(const pmc_step_t* s, const void* logp, int logp_is_f32, void* stream) {
    if (!s || !logp || !s->lik_x || !s->clean_count || !s->cur.x || !s->p_fin || !s->p_logp || s->D < 1)
        return pmc_fail("pmc_step_prior_rows: needs logp, lik_x, clean_count, cur.x, p_fin and p_logp");
    if (s->prior) return pmc_fail("pmc_step_prior_rows: with a device prior table pmc_step_pre evaluates the prior itself");
    if (!s->prior_rows) return pmc_fail("pmc_step_prior_rows: pmc_step_pre filled lik_x for a host prior (prior_rows is 0)");
    if ((uintptr_t)logp & (logp_is_f32 ? 3 : 7)) return pmc_fail("pmc_step_prior_rows: logp is not aligned to its element size");
    const int64_t n = s->n;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(prior_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logp,
                       logp_is_f32, s->cur.x, s->p_fin, s->p_logp, s->lik_x, s->clean_count, n, (int)s->D);
    return pmc_check_launch("prior_rows_kernel");
}

extern "C" int pmc_propose_inverse(int kind, const float* cur32, const double* mu, const double* inv_cov,
                                   const double* chol, double nu, double sigma, double cn_a, const pmc_rng_t* rng,
                                   double* prop64, double* quad, double* quad_prop, const pmc_maf_t* maf, float* u_out,
                                   float* ladj, int64_t n, void* stream) {
    if (!cur32 || !chol || !rng || !prop64 || !maf || !u_out || n < 0) return pmc_fail("pmc_propose_inverse: bad argument");
    if (kind == PMC_KIND_TPCN && (!mu || !inv_cov || !quad || !quad_prop))
        return pmc_fail("pmc_propose_inverse: tpCN needs mu, inv_cov and the quadratic-form outputs");
    if (n == 0) return 0;
    pmc_inverse_plan_t plan;
    if (int e = pmc_plan_inverse(maf, n, PMC_INVERSE_AUTO, PMC_FUSED_ANY, 0, 0, &plan)) return e;
    if (plan.sweep == PMC_SWEEP_NONE) return pmc_fail("pmc_propose_inverse: only the affine flows with D <= 64 have a fused instance");
    const ProposeArgs pa{kind, cur32, mu, inv_cov, chol, nu, sigma, cn_a, *rng, prop64, quad, quad_prop, nullptr};
    return pmc_launch_inverse(&plan, &pa, maf, nullptr, u_out, ladj, n, (hipStream_t)stream);
}

// what pmc_step_post asks of its device blobs, asked of any pair of blob buffers
static int blob_buffers_check(const char* who, const void* a, const void* b, int64_t row_bytes) {
    char msg[160];
    if (row_bytes < 4 || row_bytes % 4 || row_bytes > PMC_BLOB_ROW_BYTES_MAX) {
        snprintf(msg, sizeof msg, "%s: blob_row_bytes must be a multiple of 4 between 4 and PMC_BLOB_ROW_BYTES_MAX", who);
        return pmc_fail(msg);
    }
    if (((uintptr_t)a | (uintptr_t)b) & 3) { snprintf(msg, sizeof msg, "%s: blob buffers must be 4-byte aligned", who); return pmc_fail(msg); }
    if (a == b) { snprintf(msg, sizeof msg, "%s: the two blob buffers must be different buffers", who); return pmc_fail(msg); }
    return 0;
}

extern "C" int pmc_blob_rows_move(const int32_t* accept, const void* src, void* dst, int64_t n, int64_t row_bytes,
                                  void* stream) {
    if (!accept || !src || !dst || n < 0) return pmc_fail("pmc_blob_rows_move: needs accept, src, dst and n >= 0");
    if (int e = blob_buffers_check("pmc_blob_rows_move", src, dst, row_bytes)) return e;
    if (n == 0) return 0;
    blob_rows_move_launch<BLOB_MOVE_INFLIGHT>(accept, src, dst, n, (int)(row_bytes / 4), (hipStream_t)stream);
    return pmc_check_launch("blob_rows_move_kernel");
}

// blobs of a host likelihood (pmc_step_t.blob_host: blob_prop is the host's pinned buffer): the move launch behind the accept
static bool step_host_blobs(const pmc_step_t* s) { return s->blob_host != 0; }

static int step_move_host_blobs(const pmc_step_t* s, void* stream) {
    return pmc_blob_rows_move(s->accept, s->blob_prop, s->blob_cur, s->n, s->blob_row_bytes, stream);
}

// move_blobs = false: the caller enqueues the host blobs' move launch itself (the sharded pipeline: behind the exchange)
static int step_post(const pmc_step_t* s, const pmc_rng_t* rng, double beta, double nu, int want_mask, int copy_sums,
                     void* stream, bool move_blobs) {
    if (!s || !rng) return pmc_fail("pmc_step_post: null argument");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = s->n;
    pmc_rng_t rr = *rng;
    if (s->rng_ready && s->rng_uniform[0] && s->rng_uniform[1] && !rng->uniform && !rng->normal && !rng->gamma &&
        *s->rng_ready == (int64_t)rng->step + 1) {
        rr.uniform = s->rng_uniform[rng->step & 1];                      // drawn ahead of time by pmc_step_pre
        rng = &rr;
    }
    // device likelihood: logl' is in p_logl and logp' in p_logp already (the device prior, or pmc_step_lik_rows).  Unlike the
    // pre-step's, this devlik does not ask for a prior on the device: behind a host prior x' went to the host first
    // (pmc_step_lik_rows filled lik_x), but logl' is on the device all the same.
    const bool devlik = s->lik_x != nullptr;
    const int mode = step_mode(s, devlik);
    if (devlik && (!s->clean_count || !s->h_calls)) return pmc_fail("pmc_step_post: a device likelihood needs clean_count and h_calls");
    // blobs of a device likelihood (blob_cur / blob_prop): the accept launch moves the accepted rows'
    const bool blobs = !step_host_blobs(s) && s->blob_row_bytes != 0 && s->blob_cur && s->blob_prop;
    if (blobs) {
        if (!devlik) return pmc_fail("pmc_step_post: blobs on the device need a device likelihood (lik_x)");
        if (s->blob_row_bytes < 0 || s->blob_row_bytes % 4 || s->blob_row_bytes > PMC_BLOB_ROW_BYTES_MAX)
            return pmc_fail("pmc_step_post: blob_row_bytes must be a multiple of 4 between 4 and PMC_BLOB_ROW_BYTES_MAX");
        if (((uintptr_t)s->blob_cur | (uintptr_t)s->blob_prop) & 3) return pmc_fail("pmc_step_post: blob buffers must be 4-byte aligned");
        if (s->blob_cur == s->blob_prop) return pmc_fail("pmc_step_post: blob_cur and blob_prop must be different buffers");
    }
    // blobs of a host likelihood (blob_host): a launch of its own behind the accept, which is the one without blobs
    if (step_host_blobs(s)) {
        if (devlik) return pmc_fail("pmc_step_post: blob_host is for a host likelihood (lik_x is set)");
        if (!s->blob_cur || !s->blob_prop || !s->accept) return pmc_fail("pmc_step_post: blob_host needs blob_cur, blob_prop and the accept mask");
        if (int e = blob_buffers_check("pmc_step_post", s->blob_prop, s->blob_cur, s->blob_row_bytes)) return e;
    }
    // logp' is in p_logp: the device prior's table, or the flow / joint prior's stage behind the pre-step
    const bool dev_logp = s->prior || step_has_stage(s);
    if (mode == PMC_HANDOVER_COPIES) {
        if (hipMemcpyAsync(s->p_logl, s->h_logl, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
            return pmc_fail("pmc_step_post: H2D");
        if (!dev_logp &&     // with a device prior logp' never left the device
            hipMemcpyAsync(s->p_logp, s->h_logp, (size_t)n * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
            return pmc_fail("pmc_step_post: H2D");
    }
    pmc_state_t cur = s->cur;
    pmc_proposal_t prop;
    prop.theta64 = s->preconditioned ? s->p_theta64 : nullptr;
    prop.u = s->p_u; prop.x = s->p_x; prop.logdetj = s->p_logdetj;
    // host_direct: the accept kernel reads logl' (and a host-evaluated logp') from the pinned host buffers
    prop.logl = mode == PMC_HANDOVER_DIRECT ? s->h_logl : s->p_logl;
    prop.logp = (mode == PMC_HANDOVER_DIRECT && !dev_logp) ? s->h_logp : s->p_logp;
    prop.logdetj_flow = s->preconditioned ? s->p_ldjf : nullptr;
    prop.quad = s->quad; prop.quad_prop = s->p_quad;
    int rc;
    if (mode != PMC_HANDOVER_COPIES) {
        pmc_done_t dn{s->h_done ? s->h_done + 1 : nullptr, (int64_t)rng->step + 1, nullptr};
        pmc_adapt_args ad{s->adapt_state, s->adapt_state ? s->adapt_mode : 0, s->adapt_c_sigma, s->adapt_c_mu,
                          s->adapt_cap, s->adapt_n_total, {}, 0};
        if (s->adapt_n_other < 0 || s->adapt_n_other > 7) return pmc_fail("pmc_step_post: adapt_n_other out of range");
        for (int k = 0; k < s->adapt_n_other; ++k) {
            if (!s->adapt_other[k]) return pmc_fail("pmc_step_post: null adapt_other");
            ad.other[k] = s->adapt_other[k];
        }
        ad.n_other = s->adapt_n_other;
        pmc_gate_args gate{};
        if (devlik) gate = pmc_gate_args{s->p_fin, s->clean_count, (long long*)s->h_calls, (long long)n};
        pmc_blob_args blob{};
        if (blobs) blob = pmc_blob_args{(uint32_t*)s->blob_cur, (const uint32_t*)s->blob_prop, (int)(s->blob_row_bytes / 4)};
        rc = pmc_accept_adapt(s->kind, s->preconditioned, &cur, &prop, beta, nu, rng, s->alpha, s->accept, s->sums,
                              copy_sums ? s->h_sums : nullptr, (copy_sums && s->h_done) ? &dn : nullptr, s->ws, n, s->D,
                              stream, &ad, &gate, &blob);
    }
    else if (s->adapt_state && s->adapt_mode)
        return pmc_fail("pmc_step_post: adaptation on the device needs host_direct");
    else
        rc = pmc_accept(s->kind, s->preconditioned, &cur, &prop, beta, nu, rng, s->alpha, s->accept, s->sums, s->ws, n,
                        s->D, stream);
    if (rc) return rc;
    if (copy_sums && mode == PMC_HANDOVER_COPIES &&
        hipMemcpyAsync(s->h_sums, s->sums, (size_t)(s->D + 4) * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess)
        return pmc_fail("pmc_step_post: D2H sums");
    if (move_blobs && step_host_blobs(s)) {
        rc = step_move_host_blobs(s, stream);
        if (rc) return rc;
    }
    if (want_mask && s->h_accept &&
        hipMemcpyAsync(s->h_accept, s->accept, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess)
        return pmc_fail("pmc_step_post: D2H accept");
    return 0;
}

extern "C" int pmc_step_post(const pmc_step_t* s, const pmc_rng_t* rng, double beta, double nu, int want_mask,
                             int copy_sums, void* stream) {
    return step_post(s, rng, beta, nu, want_mask, copy_sums, stream, true);
}

#ifdef PMC_DEBUG_HOOKS
// measurement only (bench.py, PMC_BENCH_EPI_STAMPS, a library built with `make DEBUG_HOOKS=1`): device int64 [blocks][8] that
// the epilogue of the fused launches over n_rows rows stamps, or NULL
extern "C" void pmc_debug_set_epilogue_stamps(long long* dev, int64_t n_rows) { g_epilogue_stamps = dev; g_epilogue_stamps_n = n_rows; }
// measurement only (scripts/time_flow_prior.py --host): the C pipeline enqueues every lane's prior stage right behind that
// lane's pre-step instead of all of them behind the last lane's
extern "C" void pmc_debug_set_stage_per_lane(int on) { g_stage_per_lane = on != 0; }
#endif

extern "C" int pmc_stream_synchronize(void* stream) {
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return pmc_fail_hip(e, "hipStreamSynchronize");
    return 0;
}

// HIP events for live kernel timing from the host language (bench.py records the flow-inverse
// launch of every timed step through pmc_step_t.ev_inv0 / ev_inv1).
extern "C" void* pmc_event_create(void) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDefault) != hipSuccess) { pmc_fail("hipEventCreate failed"); return nullptr; }
    return (void*)e;
}
extern "C" int pmc_event_record(void* ev, void* stream) {
    hipError_t e = hipEventRecord((hipEvent_t)ev, (hipStream_t)stream);
    return e == hipSuccess ? 0 : pmc_fail_hip(e, "hipEventRecord");
}
// spin on a completion word the kernels store to pinned host memory (pmc_done_t)
extern "C" int pmc_wait_flag(const int64_t* flag, int64_t value, double timeout_s) {
    if (!flag) return pmc_fail("pmc_wait_flag: null flag");
    const volatile int64_t* f = flag;
    for (long it = 0;; ++it) {
        for (int k = 0; k < 2048; ++k) {
            if (*f == value) { __atomic_thread_fence(__ATOMIC_ACQUIRE); return 0; }
            __builtin_ia32_pause();
        }
        if ((it & 63) == 63) {
            static thread_local struct timespec t0;
            struct timespec t;
            clock_gettime(CLOCK_MONOTONIC, &t);
            if (it == 63) t0 = t;
            if (timeout_s > 0.0 && (double)(t.tv_sec - t0.tv_sec) + 1e-9 * (double)(t.tv_nsec - t0.tv_nsec) > timeout_s)
                return pmc_fail("pmc_wait_flag: timed out waiting for the device");
        }
    }
}

extern "C" int pmc_event_synchronize(void* ev) {
    hipError_t e = hipEventSynchronize((hipEvent_t)ev);
    return e == hipSuccess ? 0 : pmc_fail_hip(e, "hipEventSynchronize");
}
extern "C" float pmc_event_elapsed_ms(void* a, void* b) {
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, (hipEvent_t)a, (hipEvent_t)b) != hipSuccess) return -1.0f;
    return ms;
}
extern "C" void pmc_event_destroy(void* ev) { if (ev) (void)hipEventDestroy((hipEvent_t)ev); }


// ------------------------------------------------------------------------------------------------------------------
// The pipelined step of a walker set stepped as K row ranges (lanes), as ONE object behind the C ABI: the host language
// is left with the black boxes.  Per step (pocomc/mcmc.py:74-156) the driver thread does
//     pmc_pipeline_next(p, -1, ...)            wait for lane 0's x'
//     for k in lanes:  likelihood(lane k);  pmc_pipeline_next(p, k, ...)
// and every call of pmc_pipeline_next enqueues what the device can do next and returns when the host has something to
// do: the accept of lane k behind its logl', then either the wait for lane k+1's x', or -- behind the last lane -- the
// closing accept (total sums, sigma / mu update on the device, sums + completion word to the host), the pre-steps of
// step + 1 for all lanes, and the wait for the sums.  The same launches in the same order as mcmc.LanedEngine's
// step_pipelined (Python, round 2): results are bit-identical; the ~60 us of interpreter time per step are not.
struct pmc_pipeline {
    int n_lanes;
    const pmc_step_t* lanes[8];
    pmc_rng_t rng[8];
    int64_t step;                 // the step whose pre-steps are in flight
    void* stream;
    void* prefetcher;
    void* comm;                   // pmc_comm of a sharded walker set (the ranks' sums are exchanged behind the last accept), or NULL
    double timeout;
    double t_wait_x, t_wait_sums, t_enq_accept, t_enq_pre;
    int64_t n_steps;
};

static double now_s() {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

extern "C" void* pmc_pipeline_create(const pmc_step_t* const* lanes, int32_t n_lanes, uint64_t seed,
                                     const uint64_t* offsets, void* prefetcher, double wait_timeout_s, void* stream) {
    if (!lanes || n_lanes < 1 || n_lanes > 8 || !offsets) { pmc_fail("pmc_pipeline_create: 1..8 lanes"); return nullptr; }
    for (int k = 0; k < n_lanes; ++k) {
        const pmc_step_t* s = lanes[k];
        if (!s || !s->host_direct || !s->h_done || !s->done_ticket || !s->adapt_state || s->p_xT) {
            pmc_fail("pmc_pipeline_create: every lane needs host_direct buffers, completion words and adapt_state");
            return nullptr;
        }
        if (s->adapt_state != lanes[0]->adapt_state) { pmc_fail("pmc_pipeline_create: one adapt_state for all lanes"); return nullptr; }
    }
    pmc_pipeline* p = new pmc_pipeline();
    p->n_lanes = n_lanes;
    for (int k = 0; k < n_lanes; ++k) {
        p->lanes[k] = lanes[k];
        p->rng[k] = pmc_rng_t{nullptr, nullptr, nullptr, seed, 0, offsets[k]};
    }
    p->step = 0;
    p->stream = stream;
    p->prefetcher = prefetcher;
    p->comm = nullptr;
    p->timeout = wait_timeout_s;
    p->t_wait_x = p->t_wait_sums = p->t_enq_accept = p->t_enq_pre = 0.0;
    p->n_steps = 0;
    return p;
}

extern "C" void pmc_pipeline_destroy(void* pp) { delete (pmc_pipeline*)pp; }

// a sharded walker set (one process per GPU): behind the last lane's accept the ranks' sums are added by the library's own
// all-reduce (pmc_comm_adapt_update: IPC mailboxes, sums in rank order) before the adaptation -- the same pipeline as a
// single rank's, one more dependent launch
extern "C" int pmc_pipeline_set_comm(void* pp, void* comm) {
    pmc_pipeline* p = (pmc_pipeline*)pp;
    if (!p) return pmc_fail("pmc_pipeline_set_comm: null pipeline");
    p->comm = comm;
    return 0;
}

static int pipeline_enqueue_pre(pmc_pipeline* p, int64_t step, double nu) {
#ifdef PMC_DEBUG_HOOKS
    const bool stage_per_lane = g_stage_per_lane;     // (measurement: every lane's stage right behind its own pre-step)
#else
    const bool stage_per_lane = false;
#endif
    for (int k = 0; k < p->n_lanes; ++k) {
        pmc_step_ext2_t sx = step_copy(p->lanes[k]);
        pmc_step_t& s = sx.step;
        s.adapt_mode = 1;                                   // (pre: any non-zero mode = read sigma, cn_a, mu from adapt_state)
        p->rng[k].step = (uint64_t)step;
        const int rc = step_pre(&s, &p->rng[k], nu, 0.0, 0.0, p->stream, false);
        if (rc) return rc;
        if (step_has_stage(&s) && stage_per_lane) { if (int e = prior_stage_enqueue(&s, p->stream)) return e; }
        if (p->prefetcher)                                  // helper threads read x' once as soon as its completion word shows up
            (void)pmc_prefetcher_submit(p->prefetcher, s.h_done, step + 1, s.h_x, (int64_t)s.n * s.D * 8, p->timeout > 0 ? p->timeout : 1.0);
    }
    // the lanes' flow / joint prior (pmc_step_ext_t.prior_stage) behind the LAST lane's pre-step: no lane's x' waits behind
    // another lane's log_prob (profiles/step_prior.txt has both orders)
    for (int k = 0; k < p->n_lanes; ++k) {
        if (!step_has_stage(p->lanes[k]) || stage_per_lane) continue;
        const int rc = prior_stage_enqueue(p->lanes[k], p->stream);
        if (rc) return rc;
    }
    // the variates of step + 1 behind the LAST lane's pre-step: they write the other parity's buffers, nothing reads them
    // before the next step, and no lane's x' waits behind another lane's fill
    for (int k = 0; k < p->n_lanes; ++k) {
        const int rc = pmc_step_fill_next(p->lanes[k], &p->rng[k], nu, p->stream);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int pmc_pipeline_start(void* pp, double nu, int64_t first_step) {
    pmc_pipeline* p = (pmc_pipeline*)pp;
    if (!p) return pmc_fail("pmc_pipeline_start: null pipeline");
    p->step = first_step;
    return pipeline_enqueue_pre(p, first_step, nu);
}

extern "C" int pmc_pipeline_next(void* pp, int32_t lane_done, double beta, double nu, int32_t adapt_mode, double c_sigma,
                                 double c_mu, double cap, double n_total, int32_t more) {
    pmc_pipeline* p = (pmc_pipeline*)pp;
    if (!p || lane_done < -1 || lane_done >= p->n_lanes) return pmc_fail("pmc_pipeline_next: bad argument");
    const int last = p->n_lanes - 1;
    double t0 = now_s();
    if (lane_done >= 0) {
        pmc_step_ext2_t sx = step_copy(p->lanes[lane_done]);
        pmc_step_t& s = sx.step;
        s.adapt_n_other = 0;
        s.adapt_mode = 0;
        if (lane_done == last && !p->comm) {
            // the last range's accept closes the set: total sums, sigma / mu update, sums + completion word to the host
            s.adapt_mode = adapt_mode; s.adapt_c_sigma = c_sigma; s.adapt_c_mu = c_mu; s.adapt_cap = cap;
            s.adapt_n_total = n_total;
            for (int k = 0; k < last; ++k) s.adapt_other[k] = p->lanes[k]->sums;
            s.adapt_n_other = last;
        }
        // (blobs of a host likelihood: the lane's move launch follows its accept -- behind the exchange, where the exchange
        //  stores the completion word the host waits for)
        const bool exchange = lane_done == last && p->comm;
        const int rc = step_post(&s, &p->rng[lane_done], beta, nu, 0, (lane_done == last && !p->comm) ? 1 : 0, p->stream, !exchange);
        if (rc) return rc;
        if (exchange) {
            // sharded: this rank's lanes + the other ranks' totals (rank order), the adaptation, sums + completion word
            const double* parts[8];
            for (int k = 0; k <= last; ++k) parts[k] = p->lanes[k]->sums;
            const pmc_step_t* sl = p->lanes[last];
            pmc_done_t dn{sl->h_done + 1, (int64_t)p->step + 1, nullptr};
            const int rc2 = pmc_comm_adapt_update(p->comm, parts, last + 1, sl->D, nullptr, sl->h_sums, sl->adapt_state, adapt_mode,
                                                  c_sigma, c_mu, cap, n_total, &dn, p->timeout, p->stream);
            if (rc2) return rc2;
            if (step_host_blobs(&s)) {
                const int rc3 = step_move_host_blobs(&s, p->stream);
                if (rc3) return rc3;
            }
        }
        const double t1 = now_s();
        p->t_enq_accept += t1 - t0;
        t0 = t1;
    }
    if (lane_done < last) {
        // the next lane's x'
        const pmc_step_t* nx = p->lanes[lane_done + 1];
        const int rc = pmc_wait_flag(nx->h_done, p->step + 1, p->timeout);
        p->t_wait_x += now_s() - t0;
        return rc;
    }
    if (more) {
        const int rc = pipeline_enqueue_pre(p, p->step + 1, nu);
        if (rc) return rc;
        const double t1 = now_s();
        p->t_enq_pre += t1 - t0;
        t0 = t1;
    }
    const int rc = pmc_wait_flag(p->lanes[last]->h_done + 1, p->step + 1, p->timeout);
    p->t_wait_sums += now_s() - t0;
    p->step += 1;
    p->n_steps += 1;
    return rc;
}

// out[0..5] <- { seconds waiting for x', for the sums, enqueuing accepts, enqueuing pre-steps, steps, 0 } since the last reset
extern "C" int pmc_pipeline_stats(void* pp, double* out, int32_t reset) {
    pmc_pipeline* p = (pmc_pipeline*)pp;
    if (!p || !out) return pmc_fail("pmc_pipeline_stats: null argument");
    out[0] = p->t_wait_x; out[1] = p->t_wait_sums; out[2] = p->t_enq_accept; out[3] = p->t_enq_pre;
    out[4] = (double)p->n_steps; out[5] = 0.0;
    if (reset) { p->t_wait_x = p->t_wait_sums = p->t_enq_accept = p->t_enq_pre = 0.0; p->n_steps = 0; }
    return 0;
}
