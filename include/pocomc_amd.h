/* pocomc_amd -- C ABI of the MI355X (gfx950) engine for pocoMC's flow-preconditioned
 * particle MCMC step.
 *
 * The reference (minaskar/pocomc v1.2.6) has no FFI: its seam is two duck-typed
 * Python contracts:
 *   - the MCMC-kernel contract  kernel(state_dict, function_dict, option_dict)
 *     called from Sampler._mutate (pocomc/sampler.py:568-617), and
 *   - the Flow contract  forward / inverse / log_prob / sample / fit
 *     (pocomc/flow.py:99-384, pocomc/tools.py:336-349).
 * Every entry point below replaces one piece of reference arithmetic on that
 * path and cites it.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - all data pointers are DEVICE pointers to contiguous row-major arrays owned
 *     by the caller; the library allocates nothing and keeps no state between
 *     calls (except the last error string, per thread);
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work;
 *   - return 0 on success, non-zero on error; pmc_last_error() returns the text;
 *   - "f32"/"f64" in a parameter comment is the element type.  The reference
 *     keeps MCMC state in float64 numpy and the flow in float32 torch
 *     (pocomc/tools.py:279-292); so does this library.
 */
#ifndef POCOMC_AMD_H
#define POCOMC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMC_ABI_VERSION 9

const char* pmc_last_error(void);
int pmc_abi_version(void);
/* 16 hex digits: sha256 over the Makefile, the .hip and .h files of csrc/ and this header (sorted by name, concatenated) at build
 * time, "+debug" appended by DEBUG_HOOKS builds.  The Python loader recomputes it from the tree and refuses a library
 * that was not built from the sources it sits next to. */
const char* pmc_build_id(void);

/* ------------------------------------------------------------------ flow */

/* Device image of one MAF (pocomc/flow.py:55-68 -> zuko.flows.MAF).  Built by
 * the host side (pocomc_amd/maf_spec.py) and filled by pmc_maf_pack(). */
typedef struct pmc_maf {
    const float* packed;      /* packed weights, T * pk_per_transform floats */
    const int32_t* meta;      /* [8 hdr][T*D feat_of_rank][T*D rank_of_feat][nQ quad meta]; with PMC_MAF_TABLES: 16-byte aligned,
                               * [zeros up to a multiple of 4 words][the two-wave affine sweep's tables] behind them */
    int32_t D, H, T;          /* features, hidden width, transforms */
    int32_t Hp, Dp;           /* padded hidden slots / ranks (multiples of 16) */
    int32_t nT, nXT, nOT;     /* hidden, input and output tiles */
    int64_t pk_per_transform;
    int32_t tri_ok;           /* every degree group fits one 16-slot tile */
    int32_t n_out;            /* hyper-network outputs per feature: 2 = affine (MAF), 23 = 8-bin spline (NSF) */
    const uint16_t* lane16;   /* NULL, or the 16-bit image of the lane-per-walker sweep's helper fragments (pmc_maf_pack_lane16):
                               * the inverse of the wide flows then multiplies everything left of the diagonal tile with 16-bit
                               * operands and float32 accumulation -- an opt-in precision, see PMC_INVERSE_TRIANGULAR_LANE16 */
    int32_t lane16_fmt;       /* 1 bfloat16, 2 float16 (0: no image) */
    int32_t reserved;         /* 0, or PMC_MAF_VARIANT_* bits: schedule variants of the inverse sweeps that must agree with
                               * the default bit for bit (the cross-checks of tests/test_gpu_flow.py); PMC_MAF_TABLES */
} pmc_maf_t;

#define PMC_MAF_VARIANT_LEFT_LOOKING 1  /* two-wave spline sweep: the burst wave forms no output partials ahead of time */
#define PMC_MAF_VARIANT_LANE_FOUR 2     /* lane-per-walker sweep of a flow of >= 16 hidden tiles: no fifth wavefront */
#define PMC_MAF_VARIANT_LEAN_LDS 8      /* forward / D-pass workgroup kernel and float32 trainer: the instances with two hidden-width
                                         * LDS arrays (pmc_maf_lds_plan) also where the full ones fit -- a test switch, not an option */
/* meta carries the constant tables of the two-wave affine sweep (D <= 64) in the layout of the kernel's LDS, so that a
 * workgroup copies them instead of deriving them from the quad meta words and the rank maps on every launch:
 *   DGT [nT+2][16]  per hidden tile (two rows of "no groups" behind the last): words 0..3 the ranks its four degree groups
 *                   produce (D: no group; word 0 also carries the quad pattern << 16), 4..7 the byte offset of each rank's
 *                   x / y word (walker 0), 8..11 of its (shift, raw) pair in a staged output tile, 12..15 of its two rows in
 *                   an output fragment record (0x40000000 for no group)
 *   PRM [Dp]        feature of every rank of transform 0
 *   YT  [T][nT+2][4]  byte offset of the y word of the rank a group produces in the x array of transform t + 1 (by that
 *                   transform's ranks; the last transform: its own rank)
 *   Y0T [T]         the same for rank 0; zeros up to a multiple of 4 words
 * pocomc_amd/maf_spec.py (MAFSpec.sweep_tables) builds them.  Without the bit the kernel builds the same words itself. */
#define PMC_MAF_TABLES 4

#define PMC_INVERSE_AUTO 0
#define PMC_INVERSE_TRIANGULAR 1   /* one sweep over the degree groups */
#define PMC_INVERSE_NAIVE 2        /* the reference's D fixed-point passes (zuko) */
#define PMC_INVERSE_TRIANGULAR_SOLO 6 /* the D <= 64 sweep, one wavefront per 16 rows: the left-looking cross-check of the two-wave sweeps (affine and spline flows) */
#define PMC_INVERSE_TRIANGULAR_LANE 8 /* lane-per-walker chain wavefront + three or four helper wavefronts per 16-64 rows (AUTO: affine flows with >= 16 hidden tiles or D > 64) */
#define PMC_INVERSE_TRIANGULAR_LANE16 9 /* the lane-per-walker sweep with 16-bit helper operands (pmc_maf_t.lane16 required): the chain --
                                        * diagonal tiles, newest ranks, univariate map, log-determinant -- stays float32, the
                                        * left-looking products of the three helper wavefronts run on v_mfma_f32_16x16x16_bf16 / _f16
                                        * with float32 accumulation; two walker subsets share a workgroup at D = 128 (BASELINE config
                                        * 5: 5000 walkers in one round).  AUTO takes it when the image is attached and the flow is
                                        * one the lane sweep is preferred for; _LANE (8) always multiplies in float32 */
#define PMC_INVERSE_TRIANGULAR_WG 10 /* right-looking sweep of the affine flows with a workgroup of eight wavefronts per 16 rows and two
                                      * hidden-width LDS arrays (csrc/maf_inverse_wg.hip): an explicit opt-in (Flow(inverse_sweep=
                                      * "workgroup")), AUTO never takes it.  It covers every affine flow whose degree groups fit a tile
                                      * and whose arrays fit 160 KiB of LDS -- among them the default-width flows at D = 92-114, which
                                      * no other sweep fits.  Workgroup barriers only between its wavefronts, float32 throughout */
#define PMC_INVERSE_TRIANGULAR_WG_NSF 11 /* the spline counterpart (csrc/maf_inverse_wg_nsf.hip): the same workgroup of eight wavefronts per
                                          * 16 rows and two hidden-width LDS arrays, the 23 parameters of a rank by a left-looking product over
                                          * the final h2 tiles that all wavefronts share.  An explicit opt-in (Flow(inverse_sweep=
                                          * "workgroup_spline")), AUTO never takes it.  It covers every 8-bin spline flow whose degree groups
                                          * fit a tile and whose arrays fit 160 KiB of LDS -- among them the default-width flows at
                                          * D = 97-108, which no other spline sweep fits.  Affine flows do not know it */
#define PMC_INVERSE_TRIANGULAR_DUO 7  /* the same sweep with a second, burst wavefront per 16 rows, right-looking (AUTO: affine flows of < 16 hidden tiles, spline flows with D <= 64) */

/* packed[i] = idx[i] >= 0 ? flat[idx[i]] : 0   (canonical fp32 params -> kernel layout) */
int pmc_maf_pack(const float* flat, const int32_t* pack_idx, float* packed, int64_t n_packed, void* stream);

/* Flow.forward, pocomc/flow.py:99-114: data -> latent.  x,z f32 [n][D]; ladj f32 [n] or NULL;
 * log_prob f32 [n] or NULL (Flow.log_prob, flow.py:134-147). */
int pmc_maf_forward(const pmc_maf_t* m, const float* x, float* z, float* ladj, float* log_prob,
                    int64_t n, void* stream);

/* bf16 matrix-core variant of pmc_maf_forward (BASELINE config 5: "8-layer MAF bf16"), for the affine flows (n_out = 2)
 * and the spline flows of 4, 8 and 16 bins (n_out = 11, 23, 47); any other n_out is refused.
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation, the univariate map and the log-determinant in fp32 -- the spline is
 * evaluated on the unrounded fp32 x from an fp32 panel of its 3 K - 1 parameters.  The weight
 * fragments are a bf16 image of the fp32 master parameters: image u16 [T * image_per_transform], built by
 * pmc_maf_pack_bf16 through MAFSpec.pack_index_bf16 (image[i] = bf16(flat[idx[i]]) or 0; round to nearest even);
 * image_per_transform must be MAFSpec.bf16_layout's; biases are read from the fp32 image of `m`.  idx i64 [n] or NULL:
 * row gather like pmc_maf_loss_grad.  Fails with a message when one 16-row set of the flow (activations, and for a spline
 * flow n_out KB of panel) exceeds 160 KB of LDS.  There is no width rule here: Flow(precision="bf16") has one.
 * Precision: activations and weights carry 8 mantissa bits -- the parity tests state the tolerance against the fp32
 * oracle, tests/test_gpu_bf16_model.py and tests/test_gpu_bf16_spline.py hold the kernel to a model that rounds where it
 * does. */
int pmc_maf_pack_bf16(const float* flat, const int32_t* pack_idx, uint16_t* image, int64_t n, void* stream);
int pmc_maf_forward_bf16(const pmc_maf_t* m, const uint16_t* image, int64_t image_per_transform, const float* x,
                         float* z, float* ladj, float* log_prob, int64_t n, const int64_t* idx, void* stream);

/* Flow.inverse, pocomc/flow.py:116-132: latent -> data with the log-determinant of the
 * inverse map.  z,x f32 [n][D]; ladj f32 [n] or NULL. */
int pmc_maf_inverse(const pmc_maf_t* m, const float* z, float* x, float* ladj, int64_t n,
                    int algo, void* stream);
/* Which sweep PMC_INVERSE_AUTO (and with it the MCMC step) launches for this flow: 1 / 0.  _is_duo: the two-wave sweep of
 * the affine flows with D <= 64 for a call of n rows; _is_lane: the lane-per-walker sweep; _is_nsf2: the two-wave spline
 * sweep.  (bench.py names the kernel its roofline line is about with them.) */
int pmc_maf_inverse_auto_is_duo(const pmc_maf_t* m, int64_t n);
int pmc_maf_inverse_auto_is_lane(const pmc_maf_t* m);
int pmc_maf_inverse_auto_is_nsf2(const pmc_maf_t* m);

/* The whole choice behind pmc_maf_inverse and the MCMC step (csrc/inverse_plan.hip): which kernel instance a call of n
 * rows with `algo` launches for this flow.  A pure host function: it reads the descriptor's layout fields only (no
 * pointer is followed, no device is touched).
 *   sweep      PMC_SWEEP_*
 *   fused      the instance starts with the proposal (pmc_step_pre); epilogue: it ends with the scaler (+ prior)
 *   maxo       output tiles held in registers by the register-chain sweeps (4 / 8), 0 elsewhere
 *   fm         feature tiles of the fused proposal (4 / 8 / 16 quads: D <= 16 / 32 / 64), 0 unfused
 *   subsets, waves, helper_fmt   lane-per-walker sweep: walker subsets per workgroup (1 / 2 / 4), wavefronts (4 / 5),
 *              helper operands (0 float32, 1 bfloat16, 2 float16); 0 elsewhere
 *   lds_bytes  dynamic LDS of the launch
 * The descriptor is taken as one pmc_maf_inverse accepts (its consistency checks are not repeated here).
 * fused = 0: returns non-zero (pmc_last_error), with the same message, where pmc_maf_inverse refuses (flow, n, algo).
 * fused = 1: which fused proposal + inverse instance pmc_step_pre launches (algo AUTO or TRIANGULAR; the scaler taken as
 * eligible for the epilogue); sweep = PMC_SWEEP_NONE, return 0: none -- the step launches its stages one by one. */
#define PMC_SWEEP_NONE 0
#define PMC_SWEEP_DPASS_AFFINE 1
#define PMC_SWEEP_DPASS_SPLINE 2
#define PMC_SWEEP_SOLO 3
#define PMC_SWEEP_DUO 4
#define PMC_SWEEP_LANE 5
#define PMC_SWEEP_NSF_SOLO 6
#define PMC_SWEEP_NSF_DUO 7
#define PMC_SWEEP_DPASS_LEAN 8     /* the D-pass algorithm through the lean instance of the forward workgroup kernel (affine and
                                    * spline flows): AUTO / NAIVE where no sweep and no other D-pass kernel fits the LDS */
#define PMC_SWEEP_WG 9             /* the workgroup sweep (PMC_INVERSE_TRIANGULAR_WG): sweep and lds_bytes set, every other field 0 */
#define PMC_SWEEP_WG_NSF 10        /* the workgroup sweep of the spline flows (PMC_INVERSE_TRIANGULAR_WG_NSF): sweep and lds_bytes set, every other field 0 */
typedef struct pmc_inverse_plan {
    int32_t sweep, fused, epilogue, maxo, fm, subsets, waves, helper_fmt, lds_bytes;
} pmc_inverse_plan_t;
int pmc_maf_inverse_plan(const pmc_maf_t* m, int64_t n, int algo, int fused, pmc_inverse_plan_t* plan);

/* Which instance of the float32 flow kernels a flow takes, by the LDS of one workgroup (160 KiB): the forward workgroup
 * kernel (pmc_maf_forward, log_prob, pmc_maf_valid_epoch), the same kernel's D-pass inverse, and the trainer's chain kernel
 * (pmc_maf_loss_grad, pmc_maf_train_epoch).  The FULL instances keep three (trainer: four) hidden-width activation arrays
 * of 16 rows in LDS, the LEAN ones two: the forward kernel's third array aliases the first, the trainer reads the
 * activations its backward sweep gates with from the global scratch.  A flow takes the full instance wherever that fits
 * and the lean one otherwise (or with PMC_MAF_VARIANT_LEAN_LDS).  Per call: *_lean 0 / 1 and *_lds_bytes of the instance
 * taken, -1 and the full instance's bytes where neither fits (the call then fails); *_full_bytes is the full instance's
 * size whatever is taken.  forward: for the eight-wavefront launch (calls of <= 16384 rows; the four-wavefront one is 128
 * bytes smaller).  Like pmc_maf_inverse_plan a pure host function of the layout fields.  Returns non-zero (pmc_last_error:
 * the message of the first call that would fail, in the order forward, D-pass, training) where an instance is missing. */
typedef struct pmc_flow_lds_plan {
    int32_t forward_lean, forward_lds_bytes, forward_full_bytes;
    int32_t dpass_lean, dpass_lds_bytes, dpass_full_bytes;
    int32_t train_lean, train_lds_bytes, train_full_bytes;
} pmc_flow_lds_plan_t;
int pmc_maf_lds_plan(const pmc_maf_t* m, pmc_flow_lds_plan_t* plan);

/* 16-bit helper image of the lane-per-walker inverse sweep (Flow.inverse of the wide flows, flow.py:116-132, in the opt-in
 * precision of BASELINE config 5): image u16 [pmc_maf_lane16_elems(m)], derived on the device from m->packed (call again
 * after every pmc_maf_pack); fmt 1 = bfloat16, 2 = float16, round to nearest even.  Attach it as m->lane16 / lane16_fmt. */
int64_t pmc_maf_lane16_elems(const pmc_maf_t* m);
int pmc_maf_pack_lane16(const pmc_maf_t* m, int fmt, uint16_t* image, void* stream);

/* Training-side device image (host side: MAFSpec.train_index() / train_jobs()).  One minibatch is two launches:
 * a chain kernel (one workgroup per 16 rows: forward, loss, the backward sweep of the data gradients) that keeps every
 * activation and every delta of the batch in the scratch arrays below, and a weight-gradient kernel tiled over the
 * WEIGHT matrices (one workgroup per 16 x 16 tile with an unmasked entry, contracting over all rows of the batch) that
 * writes the canonical gradient -- no atomics, no per-workgroup copies of the gradient, a fixed summation order. */
typedef struct pmc_maf_train {
    const float* packedT;     /* transposed weight fragments, filled by pmc_maf_pack with the packT map */
    const int32_t* gmap;      /* canonical index of every element of a gradient tile / bias row, -1 = masked / padding */
    int64_t pkT_per_transform;
    int64_t gmap_per_transform;
    const int32_t* jobs;      /* device int32 [n_jobs][8] (MAFSpec.train_jobs): {kind_a, off_a, kind_b, off_b, gmap offset of
                               * the weight tile | -1, gmap offset of the 16 bias entries | -1, 0, 0}; kinds 0 xt_scratch,
                               * 1 act_scratch, 2 delta_scratch, 3 par_scratch; offsets in floats inside a row set's block */
    int32_t n_jobs;
    int32_t max_sets;         /* row sets of 16 the scratch arrays hold; a larger batch is taken in chunks of that many */
    int32_t n_sq_partial;     /* capacity of sq_partial, >= n_jobs */
    int32_t table_waves;      /* the wave count `tables` was built for: must equal pmc_maf_train_waves(m) */
    const int32_t* tables;    /* device int32 (MAFSpec.train_tables): [16][8] cost ranks of the hidden tiles every wave of the
                               * chain workgroup owns (-1 ends a row), [T][D] rank in transform t + 1 of the feature at rank r of
                               * transform t, [T][D] likewise for t - 1 */
    float* xt_scratch;        /* [max_sets][T + 1][Dp * 16] the input of every transform, then z */
    float* act_scratch;       /* [max_sets][T][3][Hp * 16] hidden activations h0 h1 h2 */
    float* delta_scratch;     /* [max_sets][T][3][Hp * 16] their gradients da0 da1 da2 */
    float* par_scratch;       /* [max_sets][T][par_per_transform] the hyper-network's outputs (affine: nOT tiles of (shift,
                               * raw); spline: nXT panels of 23 tiles), overwritten by their gradients */
    int64_t par_per_transform;/* floats: 256 * nOT (affine) or 256 * 23 * nXT (spline) */
    float* loss_partial;      /* [max_sets] */
    float* sq_partial;        /* [n_sq_partial] per-workgroup sums of squared gradient entries */
    const float* wsum;        /* NULL: c_n uses the sum of THIS call's weights; else f32 [1] (device) with the sum of
                               * the whole batch's weights, e.g. all-reduced over the ranks of a sharded batch */
} pmc_maf_train_t;

/* One minibatch of Flow.fit, pocomc/flow.py:297-323: loss and parameter gradient.
 *   loss += sum_n c_n * (-log_prob(x_n));  c_n = 1 (w == NULL, flow.py:309) or
 *   c_n = w_n * wmul / sum(w of the batch) (flow.py:311-312 with wmul = 1000).
 * The batch is rows idx[0..n) of x / w (idx i64 device, or NULL for rows 0..n).  x f32 [.][D];
 * grad f32 [n_params] in the canonical layout is OVERWRITTEN at every unmasked entry (masked
 * entries are never touched: allocate it zeroed); loss f32 [1] is ACCUMULATED.
 * tr->sq_partial[0 .. n_jobs) receives the sums of squares that pmc_maf_train_epoch clips with. */
/* Wavefronts per chain workgroup for this flow (16; 8 for spline flows of hidden width <= 64). */
int pmc_maf_train_waves(const pmc_maf_t* m);
int pmc_maf_loss_grad(const pmc_maf_t* m, const pmc_maf_train_t* tr, const float* x, const float* w,
                      const int64_t* idx, float wmul, float* grad, float* loss, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * bf16 matrix-core training of the wide affine flows (BASELINE config 5: D = 128, 8 transforms, H = 512; flow.py:297-323
 * with the hyper-networks of flow.py:46-90) and of the spline flows of 4 / 8 / 16 bins (m->n_out = 11 / 23 / 47).  A 512-row batch is too few rows for "one workgroup per 16 rows": the
 * layers are dense products [out x in] . [in x rows] on v_mfma_f32_16x16x32_bf16, a workgroup per 32 x 32 output tile
 * (its four wavefronts split the contraction), one launch per dependent layer (8 T + 4 per 512 rows).  fp32 master parameters, fp32
 * accumulation, fp32 univariate map / log-determinant / loss; activations and their gradients are stored as bf16 in
 * both orientations ([row][unit] feeds the next layer and the data gradients, [unit][row] the weight gradients).
 *
 * image  u16 [T * image_per_transform]: per transform, row-major and zero where masked / padded,
 *          W0f [HK][DK]  W0b = W0f^T  W1f [HK][HK]  W1b  W2f  W2b  W3f [OK][HK]  W3b
 *          with hidden units in slot order (MAFSpec.slot_unit), features in canonical order, W3 rows in canonical order
 *          n_out * feature + s ({shift, raw}; a spline: widths, heights, derivatives),
 *          DK = ceil32(D), HK = ceil32(Hp), OK = n_out * DK;
 * image_idx i32, same shape: canonical index of every element or -1 (MAFSpec.wide_index(); it is both the gather map
 *          that builds the image -- pmc_maf_pack_bf16 -- and, in its W?f parts, the scatter map of the weight gradients);
 * bias   f32 [T * bias_per_transform]: b0 b1 b2 [HK each] b3 [OK] in the same orders, bias_idx i32 likewise
 *          (pmc_maf_pack builds it);
 * scratch: pmc_maf_wide_scratch_bytes(m) bytes of device memory (a spline flow's includes its raw spline parameters in
 *          float32, T x 512 x OK floats: 36 MB at D = 128, T = 6, 8 bins); wsum as in pmc_maf_train_t.
 * A spline flow's output layer writes its parameters phi unrounded; one thread per (row, feature) evaluates the spline at
 * the unrounded x_t (forward) and its reverse mode (backward: dphi rounded to bf16, the spline's own dL/dx in float32).
 * pmc_maf_wide_refresh re-derives image and bias from the parameters (after every optimizer step). */
typedef struct pmc_maf_wide {
    uint16_t* image; const int32_t* image_idx; int64_t image_per_transform;
    float* bias; const int32_t* bias_idx; int64_t bias_per_transform;
    void* scratch; int64_t scratch_bytes;
    const float* wsum;
} pmc_maf_wide_t;
int64_t pmc_maf_wide_scratch_bytes(const pmc_maf_t* m);
int pmc_maf_wide_refresh(const pmc_maf_t* m, const pmc_maf_wide_t* wd, const float* params, void* stream);
/* Same contract as pmc_maf_loss_grad (loss accumulated, grad overwritten at the unmasked entries); dispatches on m->n_out. */
int pmc_maf_loss_grad_bf16(const pmc_maf_t* m, const pmc_maf_wide_t* wd, const float* x, const float* w,
                           const int64_t* idx, float wmul, float* grad, float* loss, int64_t n, void* stream);
/* pmc_maf_train_epoch with the bf16 loss / gradient: per batch  loss+grad -> clip -> AdamW -> refresh of the bf16 image
 * (the fp32 kernel images of opt are NOT refreshed: repack them once after the fit).  sq_scratch f32 [PMC_ADAMW_SCRATCH]. */
struct pmc_adamw;
int pmc_maf_train_epoch_bf16(const pmc_maf_t* m, const pmc_maf_wide_t* wd, struct pmc_adamw* opt, const float* x,
                             const float* w, const int64_t* perm, int64_t n, int64_t batch_size, float* loss,
                             float* sq_scratch, void* stream);

/* Optimizer state of pmc_maf_train_epoch: torch.optim.AdamW (flow.py:268) on the canonical
 * parameter vector + the two kernel images that are refreshed after every step. */
typedef struct pmc_adamw {
    float* params; float* grad; float* exp_avg; float* exp_avg_sq;
    int64_t n_params;
    const int32_t* pack_idx; float* packed; int64_t n_packed;       /* pmc_maf_t.packed */
    const int32_t* packT_idx; float* packedT; int64_t n_packedT;    /* pmc_maf_train_t.packedT */
    double lr, beta1, beta2, eps, weight_decay;
    double max_norm;          /* clip_grad_norm_ (flow.py:318); <= 0 disables */
    int64_t step;             /* optimizer steps taken so far; advanced by the call */
    /* optional inverse of pack_idx / packT_idx in CSR form: the image positions parameter i is copied to are
     * scatter_dst[scatter_ptr[i] .. scatter_ptr[i+1]), position d < n_packed in `packed`, d - n_packed in `packedT`.
     * With both non-NULL the AdamW kernel refreshes the two images itself (no separate gather launch per step). */
    const int32_t* scatter_ptr;   /* device int32 [n_params + 1] */
    const int32_t* scatter_dst;   /* device int32 [scatter_ptr[n_params]] */
    float* snapshot;              /* NULL, or device f32 [n_params]: pmc_maf_train_epoch writes the parameters behind the epoch's
                                   * LAST optimizer step there as well (the state Flow.fit restores at an early stop,
                                   * flow.py:364-374, without a separate copy launch per epoch) */
} pmc_adamw_t;

/* One epoch of the training loop, pocomc/flow.py:297-323: for every batch of `batch_size` rows
 * (rows perm[b0 .. b0+nb) of x and w, or consecutive rows when perm == NULL; the last batch may
 * be short): loss/gradient, global-norm clip, AdamW step, refresh of both kernel images.
 * loss f32 [1] accumulates the sum of the batch losses (flow.py:321).  Everything is enqueued on
 * `stream`; nothing synchronises. */
int pmc_maf_train_epoch(const pmc_maf_t* m, const pmc_maf_train_t* tr, pmc_adamw_t* opt, const float* x,
                        const float* w, const int64_t* perm, int64_t n, int64_t batch_size, float* loss,
                        void* stream);
/* The same with a gate: the epoch's first optimizer step waits for gate_event (a hipEvent_t, or NULL) -- its loss / gradient
 * launches, which only read the parameters, do not.  Lets the validation pass of the previous epoch (flow.py:327-348), which
 * reads the kernel images that step rewrites, run on another stream next to this epoch's first batch: a batch's chain kernel
 * occupies 32 of the 256 compute units. */
int pmc_maf_train_epoch_gated(const pmc_maf_t* m, const pmc_maf_train_t* tr, pmc_adamw_t* opt, const float* x,
                              const float* w, const int64_t* perm, int64_t n, int64_t batch_size, float* loss,
                              void* gate_event, void* stream);

/* Options of Flow.fit.
 * Weight regularisation, flow.py:314-315 with regularization_loss :387-421 as its docstring defines it (the function
 * itself lacks its `return`, so the reference raises TypeError when the option is set): the batch loss gains
 *   R = sum over the hyper-networks' weight matrices of |W| / laplace_scale + W^2 / (2 gaussian_scale^2)
 * (a scale <= 0 switches its term off).  loss f32 [1] += mult * R; grad (or NULL) += dR/dparams, to be called between
 * the loss/gradient of a batch and its clipped optimizer step.  is_weight u8 [n]: 1 for entries of weight matrices
 * (masked-out ones included: they are entries of zuko's `weight` parameters too), 0 for biases.
 * scratch f32 [PMC_ADAMW_SCRATCH]. */
int pmc_weight_penalty(const float* params, const uint8_t* is_weight, float* grad, int64_t n, double laplace_scale,
                       double gaussian_scale, float mult, float* loss, float* scratch, void* stream);
/* Noise augmentation, flow.py:305 / :334: out f32 [n][D] = x + scale * N(0, 1), Philox keyed by (seed, pass, row). */
int pmc_add_noise_f32(const float* x, int64_t n, int32_t D, float scale, uint64_t seed, uint64_t pass, float* out,
                      void* stream);
/* The same for rows row0 .. row0 + n of a larger set (a rank's shard of a data-parallel fit): row r draws what row
 * row0 + r of the whole set draws. */
int pmc_add_noise_rows_f32(const float* x, int64_t n, int32_t D, float scale, uint64_t seed, uint64_t pass, uint64_t row0,
                           float* out, void* stream);
/* out f32 [1] = mean_j ||x[row] - x[j]||: what flow.py:241-245 scales the noise with (its `torch.mean(min_dist)` is
 * the mean of the LAST row's distance vector, not of the nearest-neighbour distances computed above it). */
int pmc_mean_distance_f32(const float* x, int64_t n, int32_t D, int64_t row, float* out, void* stream);

/* The validation pass of one epoch, flow.py:327-348, in one call: for every batch (rows perm[b0 .. b0+nb) or
 * consecutive rows) loss += sum_n c_n * (-log_prob(x_n)) with c_n as in pmc_maf_loss_grad.
 * logp_scratch f32 [n] (one forward launch evaluates every row; the batches only shape the weight normalisation). */
int pmc_maf_valid_epoch(const pmc_maf_t* m, const float* x, const float* w, const int64_t* perm, int64_t n,
                        int64_t batch_size, float* logp_scratch, float* loss, void* stream);

/* out += sum_n -(logp_n * c_n)  (validation loss, flow.py:336-341);  out += sum_n v_n. */
int pmc_neg_weighted_sum(const float* logp, const float* w, const float* wsum, float wmul, float* out,
                         int64_t n, void* stream);
int pmc_sum_f32(const float* v, float* out, int64_t n, void* stream);

/* torch.nn.utils.clip_grad_norm_(max_norm) (flow.py:318; max_norm <= 0 disables) followed by one
 * torch.optim.AdamW step (flow.py:268, :319).  step counts from 1.
 * sq_scratch f32 [PMC_ADAMW_SCRATCH]. */
#define PMC_ADAMW_SCRATCH 256
int pmc_adamw_step(float* params, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   double lr, double beta1, double beta2, double eps, double weight_decay,
                   double max_norm, int64_t step, float* sq_scratch, void* stream);

/* ---------------------------------------------------------------- scaler */

/* pocomc/scaler.py Reparameterize with the Sampler's settings (diagonal affine,
 * scale=True; sampler.py:309-313). */
typedef struct pmc_scaler {
    const double* low;        /* [D] */
    const double* high;       /* [D] */
    const double* mu;         /* [D] */
    const double* sigma;      /* [D] */
    const int32_t* kind;      /* [D] 0 none, 1 low only, 2 high only, 3 both (scaler.py:463-489) */
    const int32_t* bc;        /* [D] bit 0 periodic, bit 1 reflective; NULL = no boundary conditions */
    const double* log_width;  /* [D] log(high-low) where kind == 3 (scaler.py:421, :424), else 0 */
    int32_t D;
    int32_t logit;            /* 0 probit, 1 logit */
    int32_t scale;            /* apply the affine part (scaler.py:219) */
    int32_t reserved;
    double sum_log_sigma;     /* sum(log(sigma)), scaler.py:306 */
} pmc_scaler_t;

/* Reparameterize.inverse (scaler.py:204-226) + the boundary-condition round trip of
 * mcmc.py:94-97 + the finite mask of mcmc.py:100-102.
 * u_in: f32 [n][D] (flow output) or NULL;  u_in64: f64 [n][D] or NULL (exactly one non-NULL)
 * u_out f64 [n][D] (u', re-derived from x' when boundary conditions apply), x f64 [n][D],
 * logdetj f64 [n], finite int32 [n] (1 = logdetj and every x finite).
 * x_colmajor: optional second copy of x as f64 [D][n] (what the host likelihood reads as an (n, D)
 * Fortran-ordered array: numpy's inner loops then run over n instead of over D), or NULL.
 * Width limit: a block keeps the Jacobian terms of its 64 rows in LDS (64 * D * 8 + 256 bytes of 160 KiB): D <= 319;
 * with x_colmajor (or the fused prior of pmc_scaler_inverse_prior) x' stays there as well (another D * 65 * 8 bytes):
 * D <= 158.  A wider call fails with "n_dim too large" before anything is launched or written. */
int pmc_scaler_inverse(const pmc_scaler_t* s, const float* u_in, const double* u_in64, double* u_out,
                       double* x, double* x_colmajor, double* logdetj, int32_t* finite, int64_t n, void* stream);

/* Reparameterize.forward (scaler.py:180-202), no input check.  x f64 [n][D] -> u f64 [n][D]. */
int pmc_scaler_forward(const pmc_scaler_t* s, const double* x, double* u, int64_t n, void* stream);

/* ----------------------------------------------------------------- prior */

/* pocomc/prior.py: a product of frozen scipy.stats distributions.  Unlike the likelihood it is not a
 * user black box: the families below are evaluated on the device, everything else stays on the host.
 * Every family is scipy's logpdf(x) = _logpdf(z; shapes) - log(scale), z = (x - loc) / scale, with scipy's support
 * test on z.  Families 1 and 2 need family / loc / scale only; the others read their shapes and constants from par
 * (rows 0-2 as listed, unlisted rows unused; row 3 log(scale)), all computed on the host in float64 with scipy.special. */
#define PMC_PRIOR_UNIFORM 1     /* scipy.stats.uniform(loc, scale) */
#define PMC_PRIOR_NORM 2        /* scipy.stats.norm(loc, scale) */
#define PMC_PRIOR_TRUNCNORM 3   /* truncnorm(a, b):    par = a, b, log-mass of [a, b] */
#define PMC_PRIOR_LOGUNIFORM 4  /* loguniform / reciprocal(a, b):  par = a, b, log(log(b) - log(a)) */
#define PMC_PRIOR_LOGNORM 5     /* lognorm(s):         par = s, 2 s^2 */
#define PMC_PRIOR_HALFNORM 6    /* halfnorm:           par = -, -, 0.5 log(2 / pi) */
#define PMC_PRIOR_EXPON 7       /* expon */
#define PMC_PRIOR_GAMMA 8       /* gamma(a):           par = a - 1, -, gammaln(a) */
#define PMC_PRIOR_INVGAMMA 9    /* invgamma(a):        par = a + 1, -, gammaln(a) */
#define PMC_PRIOR_BETA 10       /* beta(a, b):         par = a - 1, b - 1, betaln(a, b) */
#define PMC_PRIOR_CAUCHY 11     /* cauchy:             par = -, -, log(pi) */
#define PMC_PRIOR_HALFCAUCHY 12 /* halfcauchy:         par = -, -, log(2 / pi) */
#define PMC_PRIOR_LAPLACE 13    /* laplace */
#define PMC_PRIOR_T 14          /* t(df):              par = df, (df + 1) / 2, log(poch(df/2, 1/2)) - (log(df) + log(pi)) / 2;
                                   df = inf: the normal */
#define PMC_PRIOR_NPAR 4        /* rows of pmc_prior_t.par: three family constants (as above), then log(scale) */
typedef struct pmc_prior {
    const int32_t* family;    /* [D] */
    const double* loc;        /* [D] */
    const double* scale;      /* [D] */
    int32_t D;
    int32_t reserved;
    /* appended within ABI 9: families 1 and 2 ignore these */
    const double* par;        /* [PMC_PRIOR_NPAR][D] (row k of dimension j at par[k * D + j]), or NULL */
    int32_t n_extended;       /* number of factors of families 3.. : they need par, and take the scaler launch of their own
                                 in pmc_step_pre instead of the epilogue of the fused sweep */
    int32_t reserved2;
} pmc_prior_t;

/* Prior.logpdf, prior.py:70-100, with the gating of mcmc.py:105-107: logp[k] = -inf where finite[k] == 0
 * (finite may be NULL).  x f64 [n][D], logp f64 [n].  Fails when n_extended > 0 and par is NULL.  A non-finite x
 * without the mask gives a non-finite logp. */
int pmc_prior_logpdf(const pmc_prior_t* pr, const double* x, const int32_t* finite, double* logp, int64_t n,
                     void* stream);

/* Completion word of a kernel in pinned host memory: the last workgroup to finish stores `value` to `*flag`
 * after every workgroup's results are visible system-wide; the host then spins on the word (pmc_wait_flag)
 * instead of waking up through the runtime's stream / event synchronisation (~10-20 us per wait).
 * Ordering: every workgroup waits for the acknowledgement of its own stores (agent-scope release), draws a
 * ticket (agent-scope acq_rel); the last one stores the word with a system-scope release.  The results the
 * host reads behind the word must therefore live in memory the device does not cache -- pinned (coherent,
 * fine-grained) host memory, as hipHostMalloc returns it by default; the host reads the word with acquire
 * semantics (pmc_wait_flag does). */
typedef struct pmc_done {
    int64_t* flag;            /* pinned, device-accessible host memory */
    int64_t value;
    uint32_t* ticket;         /* device, zeroed once by the caller (only kernels without their own ticket use it) */
} pmc_done_t;
/* spin until *flag == value; non-zero return after timeout_s seconds */
int pmc_wait_flag(const int64_t* flag, int64_t value, double timeout_s);

/* Where the scaler (the launch of its own, or the epilogue of the fused sweep) leaves x', the finite mask and logp' next
 * to the device arrays it always writes, and how it says so.  Every field may be NULL / 0: an all-zero hand-over writes the
 * device arrays only.  pmc_step_handover returns the one pmc_step_pre uses. */
typedef struct pmc_handover {
    double* x_colmajor;       /* second copy of x' as f64 [D][n]: device (p_xT, lik_x) or pinned host (h_x) */
    int32_t* finite_copy;     /* pinned host [n] */
    double* logp_copy;        /* pinned host [n]; only with a device prior */
    uint32_t* done_ticket;    /* completion word (pmc_done_t): device ticket, ... */
    int64_t* done_flag;       /* ... pinned host word, ... */
    int64_t done_value;       /* ... and what the last workgroup stores there */
    uint32_t* bad_count;      /* device word, zero between launches: rows that do not reach the likelihood (x' or logp' not finite) */
    int64_t* bad_flag;        /* pinned host word that takes the count in front of the completion word (pmc_step_t.h_clean) */
    const double* fill_x;     /* the walkers' current x (device [n][D]): what those rows carry in x_colmajor (fill_rejected) */
} pmc_handover_t;
/* the mode that goes with a hand-over (pmc_step_handover) */
#define PMC_HANDOVER_COPIES 0
#define PMC_HANDOVER_DIRECT 1
#define PMC_HANDOVER_DEVLIK 2

/* Cache warmer for the likelihood's input (host side only; csrc/host_prefetch.hip).  n_threads helper threads, pinned to
 * cpus[i] (or unpinned when cpus == NULL) -- cores that share the L3 with the thread that calls the likelihood.  A job:
 * wait until the completion word *flag (i64, pinned host memory, written by the kernels as for pmc_wait_flag) reaches
 * value, then read buf[0 .. bytes) once, back to front, so that the likelihood finds x' in the cache hierarchy instead of
 * in DRAM.  Best effort: jobs are dropped when the helpers are more than 16 behind, a job gives up after timeout_s. */
void* pmc_prefetcher_create(int32_t n_threads, const int32_t* cpus);
int pmc_prefetcher_submit(void* prefetcher, const void* flag, int64_t value, const void* buf, int64_t bytes,
                          double timeout_s);
void pmc_prefetcher_destroy(void* prefetcher);

/* pmc_scaler_inverse and pmc_prior_logpdf in ONE launch (the step's pre-phase is a chain of small
 * latency-bound kernels; each launch costs ~15-20 us end to end): additionally
 * logp f64 [n] <- Prior.logpdf(x') on the finite rows, -inf elsewhere (mcmc.py:105-107).
 * prior == NULL and logp == NULL: exactly pmc_scaler_inverse.
 * The fused prior keeps x' in LDS like x_colmajor does: D <= 158 (pmc_scaler_inverse has the arithmetic).
 * finite_copy / logp_copy: optional second destinations.  Together with x_colmajor they may point into
 * PINNED HOST memory (device-accessible, e.g. hipHostMalloc): the kernel then writes what the host
 * callbacks read straight over PCIe while it computes, and no device-to-host copy follows it. */
int pmc_scaler_inverse_prior(const pmc_scaler_t* s, const pmc_prior_t* prior, const float* u_in,
                             const double* u_in64, double* u_out, double* x, double* x_colmajor,
                             double* logdetj, int32_t* finite, double* logp, int32_t* finite_copy,
                             double* logp_copy, const pmc_done_t* done, int64_t n, void* stream);

/* ------------------------------------------------------------ MCMC step */

#define PMC_KIND_TPCN 0   /* t-preconditioned Crank-Nicolson proposal (mcmc.py:77-85, :394-402) */
#define PMC_KIND_RWM 1    /* random-walk proposal (mcmc.py:251-253, :561-563) */

/* Random variates of one step: replay arrays (parity tests; recorded from the
 * reference's legacy numpy stream) or, when they are NULL, a counter-based
 * Philox4x32-10 keyed by (seed, step, particle). */
typedef struct pmc_rng {
    const double* gamma;      /* [n] standard-gamma draws G_k (mcmc.py:80) or NULL */
    const double* normal;     /* [n][D] N(0,1) draws (mcmc.py:85) or NULL */
    const double* uniform;    /* [n] U(0,1) draws (mcmc.py:137) or NULL */
    uint64_t seed;
    uint64_t step;
    uint64_t offset;          /* global index of this shard's first particle */
} pmc_rng_t;

/* Proposal, mcmc.py:77-85 (tpCN) / :251-253 (RWM).
 * cur32: f32 [n][D] (theta of the preconditioned kernels lives in float32, it is the
 * numpy view of a torch float32 tensor, tools.py:336-340) or NULL; cur64: f64 [n][D]
 * (u of pcn/rwm) or NULL.  mu f64 [D], inv_cov f64 [D][D], chol f64 [D][D] (lower).
 * Outputs: prop64 f64 [n][D], prop32 f32 [n][D] (what the flow consumes, tools.py:344),
 * quad f64 [n] = diff^T inv_cov diff (current), quad_prop f64 [n] (proposed); the last
 * two may be NULL for RWM.  cn_a = (1 - sigma**2)**0.5, evaluated by the caller exactly as
 * mcmc.py:85 does (ignored for RWM).
 * Width limit: D <= 128 runs on the f64 matrix cores (instances for D <= 16 / 32 / 64 / 128), 128 < D <= 157 on an
 * LDS-staged kernel (2 * D * 65 * 8 bytes of 160 KiB); D >= 158 fails with "n_dim too large" before anything is launched
 * or written. */
int pmc_propose(int kind, const float* cur32, const double* cur64, const double* mu,
                const double* inv_cov, const double* chol, double nu, double sigma, double cn_a,
                const pmc_rng_t* rng, double* prop64, float* prop32, double* quad,
                double* quad_prop, int64_t n, int32_t D, void* stream);

/* Arrays of one particle population (current or proposed). */
typedef struct pmc_state {
    float* theta32;           /* f32 [n][D] current theta (preconditioned kernels) or NULL */
    double* u;                /* f64 [n][D] */
    double* x;                /* f64 [n][D] */
    double* logdetj;          /* f64 [n] */
    double* logl;             /* f64 [n] */
    double* logp;             /* f64 [n] */
    float* logdetj_flow;      /* f32 [n] or NULL */
} pmc_state_t;

typedef struct pmc_proposal {
    const double* theta64;    /* f64 [n][D] proposed theta or NULL (pcn/rwm) */
    const double* u;          /* f64 [n][D] */
    const double* x;          /* f64 [n][D] */
    const double* logdetj;    /* f64 [n] */
    const double* logl;       /* f64 [n]  (-inf where not evaluated, mcmc.py:118) */
    const double* logp;       /* f64 [n]  (-inf where not finite, mcmc.py:107) */
    const float* logdetj_flow;/* f32 [n] or NULL */
    const double* quad;       /* f64 [n] current quadratic form (tpCN) or NULL */
    const double* quad_prop;  /* f64 [n] proposed quadratic form (tpCN) or NULL */
} pmc_proposal_t;

/* Metropolis ratio + accept + reductions: mcmc.py:124-156 (and the three variants).
 * sums f64 [D+4] <- { sum(alpha), sum(logl+logp) after accept, sum(logl+logp+logdetj) after accept,
 *                     number accepted, sum_k theta[k][0..D) after accept (cur theta32 or u) }
 * kind: PMC_KIND_TPCN adds the Student-t terms -A+B (mcmc.py:124-129); preconditioned != 0 adds the
 * flow log-determinants and moves theta (preconditioned_pcn / preconditioned_rwm), otherwise u is the
 * moved variable (pcn / rwm).
 * alpha_out f64 [n] and accept_out int32 [n] may be NULL.  workspace: pmc_accept_workspace_bytes().
 * Width limit: none for pmc_accept / pmc_accept_armed (D + 4 > 256 folds the sums in a second pass over the columns);
 * the device-side adaptation and the sums of other row ranges (pmc_step_t.adapt_*) need D <= 256 and fail above. */
int64_t pmc_accept_workspace_bytes(int64_t n, int32_t D);
int pmc_accept(int kind, int preconditioned, pmc_state_t* cur, const pmc_proposal_t* prop, double beta, double nu,
               const pmc_rng_t* rng, double* alpha_out, int32_t* accept_out, double* sums,
               void* workspace, int64_t n, int32_t D, void* stream);

/* pmc_accept without the memset that re-arms the workspace (the kernel leaves the ticket word at zero itself;
 * the caller zeroes the workspace ONCE after allocating it and never aborts a launch), and with an optional
 * second destination of the sums -- pinned host memory, so that no device-to-host copy follows the kernel.
 * prop->logl / prop->logp may likewise point into pinned host memory (read straight over PCIe). */
int pmc_accept_armed(int kind, int preconditioned, pmc_state_t* cur, const pmc_proposal_t* prop, double beta,
                     double nu, const pmc_rng_t* rng, double* alpha_out, int32_t* accept_out, double* sums,
                     double* sums_copy, const pmc_done_t* done, void* workspace, int64_t n, int32_t D, void* stream);

/* What the step needs to evaluate a flow prior (pocomc_amd.FlowPrior) or a joint prior (pocomc_amd.JointPrior) on its own
 * stream (pmc_step_ext_t.prior_stage, pmc_step_prior_stage): the descriptors the prior's own calls take and the workspaces its
 * Python class allocates for them, for the n rows of one pmc_step_t.  Everything is device memory except h_count; the
 * caller keeps all of it alive and unchanged while a step that points here is in flight. */
typedef struct pmc_prior_stage {
    const pmc_scaler_t* scaler;   /* the flow block's scaler (scaler->D = the flow's features) */
    const pmc_maf_t* maf;         /* the flow */
    const uint16_t* image16;      /* precision="bf16" flows: the bf16 image of pmc_maf_forward_bf16; NULL: pmc_maf_forward */
    int64_t image_per_transform;  /* ... and its per_t (0 without an image) */
    const int32_t* flow_cols;     /* joint prior: int32 [Df], as for pmc_joint_prior_pre; a flow prior: NULL, ... */
    const pmc_prior_t* rest;      /* ... NULL ... */
    const int32_t* rest_cols;     /* ... and NULL */
    float* u32;                   /* f32 [n][Df] */
    float* z;                     /* f32 [n][Df] (the flow writes it; not used) */
    float* lp32;                  /* f32 [n] the flow's log_prob */
    double* ldj;                  /* f64 [n] the scaler's log-determinant */
    double* rest_logp;            /* f64 [n] the table factors' sum (joint prior; a flow prior: NULL) */
    int32_t* inside;              /* int32 [n] */
    unsigned long long* count;    /* device u64 [2], zeroed once by the caller: [0] the count of the launch in flight (zero
                                   * again behind every launch), [1] the stage's launches so far */
    int64_t* h_count;             /* pinned, device-accessible host int64 [2]: word [k & 1] <- the rows of the stage's launch
                                   * number k (from 0: k = count[1]) with p_fin != 0 whose logp' is not finite.  Two words,
                                   * taken in turn: the pre-step of step k + 1 may run before the host has read the count of
                                   * step k; the host reads them in turn as well, one per step */
} pmc_prior_stage_t;

/* All buffers of one step in one place, for the composite entry points below. */
typedef struct pmc_step {
    int32_t kind;             /* PMC_KIND_TPCN | PMC_KIND_RWM */
    int32_t preconditioned;
    int64_t n;
    int32_t D;
    int32_t inverse_algo;
    const pmc_maf_t* maf;     /* NULL unless preconditioned */
    const pmc_scaler_t* scaler;
    pmc_state_t cur;          /* current population (device) */
    const double* mu;         /* device [D];  */
    const double* inv_cov;    /* device [D][D] */
    const double* chol;       /* device [D][D] */
    double* p_theta64;        /* proposal buffers (device): see pmc_propose / pmc_scaler_inverse / pmc_accept */
    float* p_theta32;
    float* p_u32;
    float* p_ldjf;
    double* p_u;
    double* p_x;
    double* p_xT;             /* optional column-major copy of x' (NULL: the host gets the row-major x') */
    double* p_logdetj;
    int32_t* p_fin;
    double* quad;
    double* p_quad;
    double* p_logl;
    double* p_logp;
    double* alpha;
    int32_t* accept;
    double* sums;             /* device [D+4] */
    void* ws;                 /* pmc_accept_workspace_bytes() */
    const double* h_mu;       /* pinned host [D] or NULL: uploaded to mu at the start of pmc_step_pre */
    double* h_x;              /* pinned host [n*D] */
    int32_t* h_fin;           /* pinned host [n] */
    const double* h_logl;     /* pinned host [n] */
    const double* h_logp;     /* pinned host [n] */
    double* h_sums;           /* pinned host [D+4] */
    int32_t* h_accept;        /* pinned host [n] or NULL */
    void* ev_inv0;            /* optional hipEvent_t recorded right before / after the flow-inverse launch */
    void* ev_inv1;
    const pmc_prior_t* prior; /* non-NULL: logp' is evaluated on the device in pmc_step_pre and copied to h_logp_out */
    double* h_logp_out;       /* pinned host [n] (may alias h_logp) */
    /* Philox variates drawn ahead of time (throughput mode, rng->normal == NULL): the draws of step k+1 do not
     * depend on step k, so pmc_step_pre(k) enqueues pmc_rng_fill(k+1) behind its own kernels and the GPU
     * generates them while the host evaluates the likelihood; the kernels of step k+1 then read them like
     * replayed variates.  Two buffer sets, used alternately; rng_ready (host int64, -1 at start) holds the step
     * whose variates sit in set [step & 1].  All NULL: the kernels draw inline. */
    double* rng_normal[2];    /* device f64 [n][D] each */
    double* rng_gamma[2];     /* device f64 [n] each (tpCN) */
    double* rng_uniform[2];   /* device f64 [n] each */
    int64_t* rng_ready;       /* host */
    void* ev_pre_done;        /* optional hipEvent_t recorded when x', finite and logp' are complete (the variates of the
                               * next step are generated behind it: wait for this event, not for the stream) */
    int64_t* h_done;          /* pinned host int64 [2] or NULL: with host_direct, [0] <- step + 1 when pmc_step_pre's results
                               * are in host memory, [1] <- step + 1 when pmc_step_post's are (pmc_wait_flag) */
    uint32_t* done_ticket;    /* device uint32 [1], zeroed once */
    int32_t no_fuse;          /* bit 0: launch the proposal and the flow inverse separately; bit 1: keep the scaler (+ prior)
                               * a launch of its own instead of the epilogue of the fused proposal + inverse launch */
    int32_t host_direct;      /* 1: h_x (column-major, p_xT == NULL), h_fin, h_logp_out and h_mu are device-accessible
                               * pinned memory that the kernels read / write themselves -- no copies in pmc_step_pre */
    /* Adaptation on the device (mcmc.py:152-156 and the variants :314-318, :476-480, :627-631): with adapt_state
     * non-NULL, pmc_step_post lets the accept kernel's last block update  {sigma, (1-sigma^2)^0.5, mu[D]}  from the
     * step's sums, and pmc_step_pre reads sigma / cn_a / mu from there instead of its arguments and h_mu -- so
     * the host can enqueue pmc_step_pre(k+1) right behind pmc_step_post(k) without waiting for the sums.  The
     * step-dependent factors are passed in (they depend on the step number only); the arithmetic keeps numpy's
     * operation order, so a host that applies the same update to the same sums holds the same sigma and mu. */
    double* adapt_state;      /* device f64 [2 + D] or NULL */
    int32_t adapt_mode;       /* PMC_ADAPT_* ; 0: the accept kernel leaves adapt_state alone */
    int32_t ext;              /* 0, or PMC_STEP_EXT: this struct is the `step` member of a pmc_step_ext_t, whose fields behind it
                               * every entry point below then reads as well (the word was reserved padding, zero in every caller
                               * so far: no offset and no size changes) */
    double adapt_c_sigma;     /* 1/(i+1)^0.75 (tpCN kinds) or 1/(i+1) (RWM kinds) of the update that follows this step */
    double adapt_c_mu;        /* 1/(i+1) */
    double adapt_cap;         /* min(2.38/sqrt(D), 0.99) */
    double adapt_n_total;     /* number of walkers the sums run over */
    const double* adapt_other[7];  /* device [D+4] sums of the other row ranges of the walker set (their accepts precede this
                               * one on the stream): added to this step's sums before the update and before the host copy */
    int32_t adapt_n_other;
    /* Blobs of a likelihood on the HOST (a vectorised host likelihood that returns (logl, blobs); the word was reserved
     * padding, zero in every caller so far: no offset and no size changes).  1: blob_cur (below) is the walkers' device
     * buffer as for a device likelihood, but blob_prop is a PINNED HOST buffer [n][blob_row_bytes] into which the host writes
     * the blobs of x' next to logl' into h_logl (rows that do not reach the likelihood may hold anything: their logl' is
     * -inf, alpha = 0).  No lik_x is needed or allowed.  pmc_step_post (and with it pmc_pipeline_next) enqueues, BEHIND the
     * accept launch on the same stream, one more launch (pmc_blob_rows_move) that reads the accept's int32 mask and copies
     * the accepted walkers' rows from blob_prop to blob_cur.  The accept launch is the one without blobs, and the move takes
     * no part in the completion words: the closing accept's word reaches the host before the move's loads cross PCIe (in a
     * sharded pipeline the move follows the exchange launch, which stores that word).
     * Ordering of the pinned buffer (one stream per lane): the host rewrites a lane's blob_prop for step k+1 only after it
     * has seen that lane's pre-step k+1 completion word (h_done[0], or ev_pre_done); that pre-step was enqueued behind the
     * lane's step-k pmc_step_post, hence behind its move launch, which has therefore read the buffer by then.  In the
     * pipeline the last lane's move launch is followed by the pre-steps of step k+1: they touch proposal buffers only --
     * neither blob_cur nor blob_prop -- so no wait is needed there either.  The walkers' blob_cur is complete once the stream
     * has been synchronised (pmc_stream_synchronize), not at the completion word h_done[1].
     * The buffers are checked as the device blobs' are (blob_row_bytes, alignment, distinct). */
    int32_t blob_host;
    /* "every row is clean": with h_clean non-NULL pmc_step_pre leaves there, before the completion word h_done[0], the
     * number of rows whose x' is not finite or whose device-evaluated logp' is not finite (mcmc.py:100-109's two masks) --
     * 0 lets the host skip both mask scans and hand the whole block to the likelihood.  -1: the launch sequence that ran
     * does not count (no device prior, or x' not handed over by the kernels); the host then scans h_fin / logp' as before. */
    int64_t* h_clean;         /* pinned host int64 [1] or NULL */
    uint32_t* clean_count;    /* device uint32 [1], zeroed once by the caller */
    /* 1: in the HOST copy of x' (h_x with host_direct) a row that does not reach the likelihood -- x' or the device-evaluated
     * logp' not finite, the rows h_clean counts -- carries the walker's current x (cur.x) instead of x'.  The host can then
     * hand the whole block to a row-wise likelihood and overwrite those rows' values with -inf (mcmc.py:118-121 does that to
     * the rows it left out) instead of gathering the other rows first (x'[mask], mcmc.py:117: 280 us for 6.5e3 x 50 doubles).
     * The device copy p_x keeps x'.  Needs h_clean / clean_count and a device prior. */
    int32_t fill_rejected;
    /* A prior that is a GPU callable of the caller's, like the likelihood (lik_x non-NULL, prior == NULL, prior_rows = 1;
     * the word was reserved padding, zero in every caller so far: no offset and no size changes):
     *   pmc_step_pre writes x' into lik_x as it does with a device prior table, but the only gate it knows is the finite
     *   mask: a row whose x' (or logdetj') is not finite carries the walker's current x and is counted in clean_count;
     *   p_fin is written, nothing goes to pinned host memory, no completion word is stored.
     *   The caller evaluates its prior on lik_x (every row; the values of the rows above are dropped) on the same stream,
     *   pmc_step_prior_rows moves the values into p_logp and closes the gate of mcmc.py:108-109, then the likelihood runs
     *   on lik_x as before.  pmc_step_post is unchanged.
     * 0: a prior the device does not evaluate is called on the host (pmc_step_lik_rows). */
    int32_t prior_rows;
    /* Likelihood on the device (mcmc.py:99-121 with the user's likelihood a GPU callable): with lik_x non-NULL x' is never
     * copied to the host and logl' never uploaded.
     *   pmc_step_pre writes x' into lik_x, column-major ((n, D) with strides (1, n)), with the walker's current x (cur.x) in
     *   every row that does not reach the likelihood -- x' or logdetj' not finite, or the device-evaluated logp' not finite
     *   (the finite_mask of mcmc.py:99-109) -- and counts those rows in clean_count (device word, zero between steps); no
     *   completion word, no copy to the host.  Without a device prior it hands x' and the finite mask to the host as before
     *   (for Prior.logpdf only); pmc_step_lik_rows then uploads the host's logp' and fills lik_x and the count.
     *   The caller evaluates the likelihood on lik_x into p_logl (device) on the same stream.
     *   pmc_step_post reads logl' from p_logl and logp' from p_logp (no H2D) and gates logl' to -inf wherever p_fin is 0 or
     *   logp' is not finite (mcmc.py:118-121) before the ratio of mcmc.py:124-134: accepted rows store the gated value; a
     *   NaN from the likelihood gives alpha = 0 (:134).  Its last block writes n - clean_count, the number of rows that
     *   reached the likelihood (mcmc.py:121's n_calls increment), to h_calls ahead of the sums and the completion word
     *   h_done[1], and zeroes clean_count.  Needs clean_count and h_calls; adapt_state is optional as for the host path.
     * Walkers row-sharded over ranks (one process per GPU), everything on one stream: pmc_step_post with adapt_mode = 0 and
     * copy_sums = 0 -- this rank's sums stay in `sums`, no adaptation, no completion word, but h_calls is still written
     * and clean_count still zeroed by that launch (the gate does not depend on a completion word being asked for) -- then
     * pmc_comm_adapt_update (or the process group's all-reduce + pmc_adapt_update) with `sums` as its single part, h_sums
     * as the host copy of the GLOBAL sums and h_done[1] as its completion word, then the next pmc_step_pre.  The count is
     * NOT moved into the exchange kernel: the accept launch completes, its stores to pinned host memory included, before
     * the exchange launch starts on the same stream, so the host reads h_calls (this rank's rows) once it has seen the
     * exchange's completion word, and not before. */
    double* lik_x;            /* device f64 [D][n] or NULL */
    int64_t* h_calls;         /* pinned host int64 [1] */
    /* Blobs of a likelihood on the device (the derived quantities a likelihood returns next to logl, mcmc.py:112-121 and
     * :139: `blobs[mask] = blobs_prime[mask]`): each walker owns one row of blob_row_bytes bytes of any content -- the
     * kernels move bytes, the caller knows the element type.  With lik_x and both pointers non-NULL and blob_row_bytes > 0,
     *   the caller's likelihood writes the blobs of x' into blob_prop on the same stream as logl' into p_logl (all n rows:
     *   the rows that did not reach the likelihood hold whatever it returned for the walker's current x);
     *   pmc_step_post's accept launch copies blob_prop's row to blob_cur for every ACCEPTED walker, in the same launch
     *   that moves u, x and theta -- no further launch, no mask on the host.  A rejected walker's row is neither read nor
     *   written: rows the gate set to -inf and a NaN logl' have alpha = 0 (:134), so their blobs never move.
     * Both buffers are device memory: the kernel boundary orders the copy for the next launch on the stream; the blobs take
     * no part in the completion words.  blob_row_bytes is a multiple of 4, at most PMC_BLOB_ROW_BYTES_MAX; the buffers are
     * 4-byte aligned and distinct.  Zero / NULL: no blobs, and the accept launch is the one without them.  pmc_accept and
     * pmc_accept_armed take no blobs. */
    void* blob_cur;           /* device [n][blob_row_bytes] or NULL */
    const void* blob_prop;    /* device [n][blob_row_bytes] or NULL (blob_host: pinned host memory, see there) */
    int64_t blob_row_bytes;
} pmc_step_t;

#define PMC_BLOB_ROW_BYTES_MAX (1 << 20)

/* pmc_step_t with fields behind it.  pmc_step_t keeps its size -- callers that allocate one pass it as ever --, so what a
 * step gains from here on is appended to this struct instead: a caller that wants it allocates a pmc_step_ext_t, sets
 * step.ext = PMC_STEP_EXT and passes &ext.step wherever a pmc_step_t* is taken (pmc_pipeline_create included).  With
 * step.ext == 0 nothing behind the pmc_step_t is read.
 *
 * prior_stage: a flow prior or a joint prior inside the step of a HOST likelihood (NULL: none, and every call does what it
 * did).  With prior_stage non-NULL and prior == NULL, prior_rows == 0, lik_x == NULL:
 *   pmc_step_pre enqueues pmc_step_prior_stage behind its own launches and copies: the prior's three launches read p_x
 *   and write p_logp on the step's stream while the host, which got x' and the finite mask exactly as for a host prior
 *   (pmc_step_handover returns what it returns without the stage), evaluates the likelihood.  Nothing about logp' goes
 *   to the host: it masks on the finite flags only.
 *   pmc_step_post takes logp' from p_logp in every hand-over mode (no H2D copy of h_logp, no read of it over PCIe).
 * A row with a finite x' whose logp' is -inf reaches the host likelihood all the same; its logl' is dropped, alpha = 0
 * through logp' (mcmc.py:130-134).  pmc_prior_stage_t.h_count tells the host how many such rows a step had. */
#define PMC_STEP_EXT 1
typedef struct pmc_step_ext {
    pmc_step_t step;
    const pmc_prior_stage_t* prior_stage;
} pmc_step_ext_t;

/* dst[r] <- src[r] (rows of row_bytes bytes) for every r < n with accept[r] != 0; the other rows are neither read nor
 * written.  accept: device int32 [n] (pmc_step_t.accept); src: device-accessible memory, typically pinned host memory
 * (the loads cross PCIe: the kernel keeps several in flight per thread); dst: device.  row_bytes a multiple of 4 between 4
 * and PMC_BLOB_ROW_BYTES_MAX, src and dst 4-byte aligned and distinct.  One launch on `stream`, no wait, no completion word. */
int pmc_blob_rows_move(const int32_t* accept, const void* src, void* dst, int64_t n, int64_t row_bytes, void* stream);

#define PMC_ADAPT_TPCN 1      /* sigma <- |min(sigma + c (mean alpha - 0.234), cap)|      (mcmc.py:152, :476) */
#define PMC_ADAPT_PRWM 2      /* sigma <- sigma + c (mean alpha - 0.234)                   (mcmc.py:314) */
#define PMC_ADAPT_RWM 3       /* sigma <- |sigma + c (mean alpha - 0.234)|                 (mcmc.py:627) */
#define PMC_ADAPT_MU 8        /* or-ed in: mu <- mu + c_mu (float32(mean theta) - mu)      (mcmc.py:156) */

/* The Philox variates of one step into arrays, exactly the values the kernels draw inline for the same
 * (seed, step, offset): normal f64 [n][D] (stream 1, pair j/2), gamma f64 [n] = standard gamma of shape
 * `gamma_shape` (stream 0; NULL or gamma_shape <= 0: skipped), uniform f64 [n] (stream 2; NULL: skipped). */
int pmc_rng_fill(const pmc_rng_t* rng, double gamma_shape, double* normal, double* gamma, double* uniform,
                 int64_t n, int32_t D, void* stream);
int pmc_event_synchronize(void* ev);

/* Proposal (pmc_propose, preconditioned kernels: cur32 = theta) and flow inverse (pmc_maf_inverse) of the
 * proposed theta' in ONE launch: every wave proposes for its 16 walkers and sweeps them through the inverse
 * flow without a global round trip.  prop64 f64 [n][D] = theta', quad / quad_prop f64 [n] (tpCN),
 * u_out f32 [n][D], ladj f32 [n] or NULL.  Affine flows with D <= 64 only (error otherwise). */
int pmc_propose_inverse(int kind, const float* cur32, const double* mu, const double* inv_cov, const double* chol,
                        double nu, double sigma, double cn_a, const pmc_rng_t* rng, double* prop64, double* quad,
                        double* quad_prop, const pmc_maf_t* maf, float* u_out, float* ladj, int64_t n, void* stream);

/* mcmc.py:77-102 in one call: [H2D mu] -> propose -> flow inverse -> scaler inverse -> D2H x', finite. */
int pmc_step_pre(const pmc_step_t* s, const pmc_rng_t* rng, double nu, double sigma, double cn_a, void* stream);
/* pmc_step_pre in two parts, for a caller that enqueues the pre-steps of several row ranges back to back (pmc_pipeline
 * does): pmc_step_pre_deferred is pmc_step_pre without the variates of step rng->step + 1 (pmc_step_t.rng_normal), which
 * pmc_step_fill_next enqueues (and notes in *rng_ready) -- behind the last range's pre-step, so that no range's x' waits
 * behind another range's fill.  pmc_step_fill_next does nothing when the step draws inline.  Every pmc_step_pre_deferred
 * needs its pmc_step_fill_next before the same range's pmc_step_post. */
int pmc_step_pre_deferred(const pmc_step_t* s, const pmc_rng_t* rng, double nu, double sigma, double cn_a, void* stream);
int pmc_step_fill_next(const pmc_step_t* s, const pmc_rng_t* rng, double nu, void* stream);
/* What pmc_step_pre of step number `step` decides about the hand-over of x', the finite mask, logp', the row count and the
 * completion word (epilogue: 1 when the fused sweep's epilogue runs the scaler, 0 for the scaler launch of its own):
 *   *out            what the scaler is given;
 *   *mode           PMC_HANDOVER_COPIES: device arrays only, then D2H copies on the stream -- logp' (with a device prior), x'
 *                   (p_xT, or p_x without one) and the finite mask;  _DIRECT: the kernels write pinned host memory, no copy;
 *                   _DEVLIK: x' into lik_x, nothing to the host;
 *   *clean_unknown  1: pmc_step_pre sets *h_clean = -1, the launch sequence does not count.
 * Host logic only: reads the fields of *s, follows none of its pointers. */
int pmc_step_handover(const pmc_step_t* s, int64_t step, int32_t epilogue, pmc_handover_t* out, int32_t* mode,
                      int32_t* clean_unknown);
/* mcmc.py:124-156 in one call: H2D logl', logp' -> accept + reductions -> [D2H sums, accept mask]. */
int pmc_step_post(const pmc_step_t* s, const pmc_rng_t* rng, double beta, double nu, int want_mask,
                  int copy_sums, void* stream);
/* Device likelihood with a prior the device does not evaluate (pmc_step_t.lik_x, prior == NULL): behind the host's
 * Prior.logpdf of the finite rows (mcmc.py:105-107, into h_logp), H2D logp' -> p_logp, then lik_x <- x' or, for the rows
 * that do not reach the likelihood (p_fin 0 or logp' not finite, mcmc.py:108-109), the walker's current x; those rows
 * are added to clean_count. */
int pmc_step_lik_rows(const pmc_step_t* s, void* stream);
/* Device likelihood with a prior that is a GPU callable (pmc_step_t.prior_rows): behind the caller's prior on lik_x, whose
 * values are in `logp` (device [n], float64, or float32 with logp_is_f32 != 0: widened here),
 *   p_logp[r] = logp[r] where p_fin[r], -inf where not (mcmc.py:105-107; a NaN is stored as it came),
 * and where p_fin[r] holds but logp[r] is not finite (mcmc.py:108-109) row r of lik_x is overwritten with the walker's
 * current x and added to clean_count, so that pmc_step_post's h_calls = n - clean_count stays "rows that reached the
 * likelihood".  One launch on `stream`: no copy, no wait. */
int pmc_step_prior_rows(const pmc_step_t* s, const void* logp, int logp_is_f32, void* stream);
/* Host likelihood with a flow prior or a joint prior on the step's stream (pmc_step_ext_t.prior_stage): three launches on
 * `stream`, behind the pre-step that wrote p_x (C-contiguous [n][D]) and p_fin -- no copy, no wait:
 *   1. pmc_flow_prior_pre (flow_cols == NULL) or pmc_joint_prior_pre on p_x;
 *   2. the flow's forward call with log_prob on u32: pmc_maf_forward, or pmc_maf_forward_bf16 with image16;
 *   3. a closing kernel:  p_logp[r] = what pmc_flow_prior_post / pmc_joint_prior_post give for the row, in the same
 *      operations and order (bit for bit), where p_fin[r] != 0, and -inf where it is 0 (mcmc.py:105-107).  It counts the
 *      rows with p_fin[r] != 0 whose logp' is not finite -- rows the host hands to the likelihood and the reference would
 *      not (mcmc.py:108-109) -- with one atomic per block; the last block stores the count to the host word whose turn it is
 *      (pmc_prior_stage_t.h_count) and zeroes the device word.  The launch completes, that store
 *      included, before the accept that follows it on the stream starts: the count is in host memory in front of the
 *      accept's completion word, and in front of the end of its copies.
 * pmc_step_pre calls it at its end; pmc_step_pre_deferred does not: pmc_pipeline_start / pmc_pipeline_next enqueue every
 * lane's stage behind the LAST lane's pre-step (no lane's x' waits behind another lane's log_prob), in front of the
 * variates of the next step.
 * Refused before anything is launched, each with a text of its own: a struct without prior_stage; with prior, prior_rows or
 * lik_x set as well; NULL descriptors, workspaces or count words; n < 1; p_x, p_fin or p_logp missing; a width that
 * pmc_flow_prior_pre / pmc_joint_prior_pre refuses (their checks, their texts) or that is not the step's D.
 * A struct announced as pmc_step_ext2_t (below, ext = PMC_STEP_EXT2) with blocks_stage set: the same place on the stream
 * and the same count protocol for the blocks form of the joint prior -- pmc_joint_blocks_pre on p_x, the blocks' forward
 * calls in block order, a closing kernel with pmc_joint_blocks_post's join; see pmc_step_ext2_t for its refusals. */
int pmc_step_prior_stage(const pmc_step_t* s, void* stream);
/* The adaptation of pmc_step_t.adapt_state as a launch of its own, for walker sets whose sums come in parts
 * (row ranges stepped one after the other, mcmc.LanedEngine; ranks, after the all-reduce):
 *   total[j] = parts[0][j] + parts[1][j] + ...   (j < D + 4, n_parts <= 8, added in this order)
 * -> total_out (device, may be NULL) and h_sums (pinned host, may be NULL); then, if adapt_state != NULL, the
 * update selected by adapt_mode (PMC_ADAPT_*) with the factors of pmc_step_t.adapt_*; finally done->flag. */
int pmc_adapt_update(const double* const* parts, int32_t n_parts, int32_t D, double* total_out, double* h_sums,
                     double* adapt_state, int32_t adapt_mode, double c_sigma, double c_mu, double cap, double n_total,
                     const pmc_done_t* done, void* stream);
int pmc_stream_synchronize(void* stream);

/* The all-reduce of a sharded step (one exchange of D + 4 doubles per step so that sigma, mu and the stop
 * decision of mcmc.py:152-180 are global) inside this library: one process per GPU on one node, a mailbox per rank in its
 * HBM shared through hipIpc handles (xGMI peer stores + sequence words), sums formed in RANK ORDER by every rank -- the same
 * bits everywhere, whatever the arrival order.
 *   comm = pmc_comm_create(rank, world <= 8, width >= D + 4);  pmc_comm_handle(comm, h64) -> 64 bytes the host language
 *   exchanges between the ranks' processes (e.g. torch.distributed.all_gather_object);  pmc_comm_connect(comm, world x 64 B).
 *   pmc_comm_adapt_update = pmc_adapt_update with the parts' total summed over the ranks first (every rank calls it in
 *   the same order; timeout_s bounds the wait for a peer: on a timeout sums[0] is NaN and `done` is written all the same).
 *   pmc_pipeline_set_comm(pipeline, comm): the pipelined step of a sharded walker set.
 * pmc_comm_create fails (NULL) where the device cannot give it UNCACHED memory -- the protocol is only valid for mailboxes
 * no device caches.  pmc_comm_create_host: the same communicator with the mailboxes in pinned, coherent HOST memory (a
 * POSIX shared-memory object per rank, registered with every rank's HIP runtime; the 64-byte handle is its name): every
 * store and poll crosses PCIe instead of xGMI -- the tier for nodes without hipIpc peer mappings, slower, same bits.  All
 * ranks of a communicator are of one kind (pmc_comm_kind: 0 device, 1 host). */
void* pmc_comm_create(int32_t rank, int32_t world, int32_t width);
void* pmc_comm_create_host(int32_t rank, int32_t world, int32_t width);
int pmc_comm_kind(void* comm);
/* host mailboxes: drop the shared-memory NAME once every rank has connected (mappings stay valid; nothing is left in /dev/shm
 * if a process dies later); no-op for device mailboxes */
int pmc_comm_unlink(void* comm);
int pmc_comm_handle(void* comm, void* out64);
int pmc_comm_connect(void* comm, const void* handles);
void pmc_comm_destroy(void* comm);
int pmc_comm_adapt_update(void* comm, const double* const* parts, int32_t n_parts, int32_t D, double* total_out, double* h_sums,
                          double* adapt_state, int32_t adapt_mode, double c_sigma, double c_mu, double cap, double n_total,
                          const pmc_done_t* done, double timeout_s, void* stream);
int pmc_pipeline_set_comm(void* pipeline, void* comm);

/* The pipelined step of a walker set stepped as row ranges ("lanes": the device works on the proposals of lane k+1 and
 * the accept of lane k-1 while the host evaluates the likelihood of lane k), as one object: everything of a loop iteration
 * of pocomc/mcmc.py:74-156 that is not a black box is enqueued by these calls; the host language keeps the prior /
 * likelihood callbacks and the stop rule (mcmc.py:159-180, from the sums in the last lane's h_sums).
 *   lanes[k]: the lanes' pmc_step_t (kept alive and unchanged by the caller; host_direct, h_done, done_ticket, rng_* set;
 *   ONE adapt_state shared by all lanes, initialised by the caller with {sigma, (1 - sigma^2)^0.5, mu}); offsets[k]: the
 *   lane's first global walker index (Philox key).
 * pmc_pipeline_start enqueues the pre-steps (pmc_step_pre) of step `first_step` for every lane.  Then, per step:
 *   pmc_pipeline_next(p, -1, ...)   returns when lane 0's x', finite mask and logp' are in host memory;
 *   pmc_pipeline_next(p, k, ...)    the host has written lane k's logl' (and a host prior's logp'): enqueues its accept
 *                                   (pmc_step_post); k < last: returns when lane k+1's x' is there; k == last: that accept
 *                                   adds the lanes' sums and applies the adaptation (adapt_mode, c_sigma, c_mu, cap, n_total
 *                                   as in pmc_step_t.adapt_*), the pre-steps of step + 1 follow (more != 0), and the call
 *                                   returns when the sums are in the last lane's h_sums.
 * Same launches in the same order as one pmc_step_pre / pmc_step_post per lane from the host language. */
void* pmc_pipeline_create(const pmc_step_t* const* lanes, int32_t n_lanes, uint64_t seed, const uint64_t* offsets,
                          void* prefetcher, double wait_timeout_s, void* stream);
void pmc_pipeline_destroy(void* pipeline);
int pmc_pipeline_start(void* pipeline, double nu, int64_t first_step);
int pmc_pipeline_next(void* pipeline, int32_t lane_done, double beta, double nu, int32_t adapt_mode, double c_sigma,
                      double c_mu, double cap, double n_total, int32_t more);
/* out f64 [6] <- { seconds spent waiting for x', waiting for the sums, enqueuing accepts, enqueuing pre-steps, steps, 0 } */
int pmc_pipeline_stats(void* pipeline, double* out, int32_t reset);
/* hipEvent helpers for the host language (live kernel timing inside bench.py). */
void* pmc_event_create(void);
int pmc_event_record(void* ev, void* stream);
float pmc_event_elapsed_ms(void* a, void* b);
void pmc_event_destroy(void* ev);

/* --------------------------------------------------------- particle math */

/* Particles.compute_logw_and_logz, particles.py:215-231, un-normalised part:
 * logw[t*N+k] = logl[t][k]*beta_final - (logsumexp_i(logl[t][k]*beta[i]-logz[i]) - log T). */
int pmc_logw(const double* logl, const double* beta, const double* logz, double beta_final,
             double* logw, int32_t T, int64_t N, void* stream);

/* stats f64 [4] <- { max(logw), sum exp(logw-max), sum exp(2(logw-max)), sum 1-(1-w)^k }  with
 * w = exp(logw-max)/sum: everything effective_sample_size / unique_sample_size /
 * increment_logz need (tools.py:56-133).  k <= 0 skips the last entry.
 * workspace: pmc_reduce_workspace_bytes(P). */
int64_t pmc_reduce_workspace_bytes(int64_t P);
int pmc_logw_stats(const double* logw, int64_t P, int64_t k, double* stats, void* workspace, void* stream);

/* trim_weights, tools.py:10-53: the weight threshold the reference's downward percentile scan stops at.
 * w f64 [P] (normalised; not modified); result f64 [2] <- { threshold, index of the accepted percentile bin };
 * the caller keeps the samples with w >= threshold (tools.py:38-39).  One radix sort + two scans
 * instead of up to `bins` np.percentile passes.  workspace: pmc_trim_workspace_bytes(P). */
int64_t pmc_trim_workspace_bytes(int64_t P);
int pmc_trim_threshold(const double* w, int64_t P, double ess, int32_t bins, double* result,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ---- SMC bookkeeping on a pool that stays in HBM (csrc/pool.hip) ------------------------------------------------ */

/* Importance weights of Sampler._reweight, sampler.py:779-781: w = exp(logw - max) / sum.
 * stats f64 [>= 2] on the device: { max, sum exp(logw - max) } as left by pmc_logw_stats. */
int pmc_weights_from_logw(const double* logw, int64_t P, const double* stats, double* w, void* stream);

/* out f64 [1] (device) <- sum of a f64 [n], added in a fixed order (np.sum of a weight vector: tools.py:34, :168). */
int pmc_sum_f64(const double* a, int64_t n, double* out, void* stream);

/* trim_weights, tools.py:38-41, after pmc_trim_threshold: keep the samples with w >= *threshold in their order,
 * idx_out i64 [<= P] <- their indices, w_out f64 [<= P] <- their renormalised weights, count i64 [1] <- how many
 * (threshold, count: device memory).  workspace: pmc_trim_select_workspace_bytes(P). */
int64_t pmc_trim_select_workspace_bytes(int64_t P);
int pmc_trim_select(const double* w, int64_t P, const double* threshold, int64_t* idx_out, double* w_out,
                    int64_t* count, void* workspace, int64_t workspace_bytes, void* stream);

/* First and second moments of the rows x[idx[r]], r < n (idx NULL: rows 0..n-1), with weights w (NULL: ones):
 * v f64 [2] <- { V1 = sum w, V2 = sum w^2 }, mean f64 [D] <- sum w x / V1, S f64 [D][D] <- sum w (x - mean)(x - mean)^T.
 * Everything np.average / np.cov(aweights=w) / np.var of Geometry.fit (geometry.py:44-49) and the start values of
 * fit_mvstud (student.py:46-47) need.  Rows float64 (x) or float32 (x32: theta, the float32 output of the flow).
 * Ordered reductions.  workspace: pmc_moments_workspace_bytes(D). */
int64_t pmc_moments_workspace_bytes(int32_t D);
int pmc_moments(const double* x, const float* x32, const int64_t* idx, const double* w, int64_t n, int32_t D,
                double* mean, double* S, double* v, void* workspace, int64_t workspace_bytes, void* stream);

/* np.median(data, 1) of student.py:45 over the rows x[idx[r]] (idx NULL: rows 0..n-1): one segmented radix sort;
 * for an even n the mean of the two middle elements in the input's precision (np.mean of a float32 pair is a
 * float32).  med64 f64 [D] for float64 rows, med32 f32 [D] for float32 rows.
 * workspace: pmc_column_medians_workspace_bytes(n, D, is_f32). */
int64_t pmc_column_medians_workspace_bytes(int64_t n, int32_t D, int32_t is_f32);
int pmc_column_medians(const double* x, const float* x32, const int64_t* idx, int64_t n, int32_t D, double* med64,
                       float* med32, void* workspace, int64_t workspace_bytes, void* stream);

/* The EM fit of a multivariate Student-t (location, scatter, degrees of freedom: what student.py:53-85 sets out to do) to
 * the rows x[idx[r]], r < n (idx NULL: rows 0..n-1; rows float64 (x) or float32 (x32), widened on load), all in float64:
 *   start: mu_io f64 [D], sigma_io f64 [D][D] as given (device), nu = 20, last_nu = 0; i = 0
 *   while |last_nu - nu| > tol and i < max_iter:      (++i)
 *     d_r = x_r - mu, delta_r = d_r^T Sigma^-1 d_r    (Cholesky factor of Sigma by one workgroup, then one lane per row)
 *     last_nu = nu; nu <- root of
 *         f(nu) = log(nu/2) - psi(nu/2) + mean(log w - w) + 1 + psi((nu+D)/2) - log((nu+D)/2),  w_r = (nu+D)/(nu+delta_r)
 *       in [PMC_STUDENT_NU_LO, PMC_STUDENT_NU_HI] = [0.1, 1e4]: f(NU_HI) >= 0 -> nu = inf, stop, mu / Sigma as they are;
 *       f(NU_LO) <= 0 -> nu = NU_LO; else a bracketed secant in log nu until the bracket is below 1e-13
 *     Sigma <- sum_r w_r d_r d_r^T / n  (w at the new nu, d about the old mu);  mu <- sum_r w_r x_r / sum_r w_r
 * mu_io / sigma_io hold the result (device).  result: HOST f64 [4] <- { nu (inf possible), iterations i, status
 * (PMC_STUDENT_*), number of host reads }.  Every reduction has a fixed order (the same bits on every call and every
 * device); convergence is decided on the device -- a done word in the workspace turns every later kernel of the call
 * into a no-op -- and the host enqueues 8 iterations at a time and reads the 32-byte state in between (the call
 * synchronises `stream`).  A Cholesky pivot that is <= 0 or not finite ends the fit with PMC_STUDENT_NOT_PD, a NaN in
 * f with PMC_STUDENT_NONFINITE: mu_io / sigma_io then hold the last completed iteration's values.
 * 1 <= D <= PMC_STUDENT_MAX_D (the packed factor and 64 rows' substitution vectors share the LDS), n > D, max_iter >= 1.
 * workspace: pmc_student_em_workspace_bytes(n, D). */
#define PMC_STUDENT_MAX_D 128
#define PMC_STUDENT_NU_LO 0.1
#define PMC_STUDENT_NU_HI 1e4
#define PMC_STUDENT_CONVERGED 0
#define PMC_STUDENT_MAX_ITER 1
#define PMC_STUDENT_NU_INF 2
#define PMC_STUDENT_LOWER_CLAMP 3   /* converged or out of iterations with nu == PMC_STUDENT_NU_LO */
#define PMC_STUDENT_NOT_PD 4
#define PMC_STUDENT_NONFINITE 5
int64_t pmc_student_em_workspace_bytes(int64_t n, int32_t D);
int pmc_student_em(const double* x, const float* x32, const int64_t* idx, int64_t n, int32_t D, double* mu_io,
                   double* sigma_io, double tol, int32_t max_iter, double* result, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* The same fit with a weight per row, w f64 [n] (device), w_r >= 0, not necessarily normalised; rows 0..n-1 (no idx), for
 * the whole width of the MCMC step.  With P = { r : w_r > 0 }, W = sum_P w_r and pi_r = w_r / W the iteration of
 * pmc_student_em reads
 *     f(nu) = [log(nu/2) - psi(nu/2)] - [log((nu+D)/2) - psi((nu+D)/2)] + sum_P pi_r (log w_r - w_r + 1)    (w_r as above)
 *     Sigma <- sum_P pi_r w_r d_r d_r^T   (no division by n);   mu <- sum_P pi_r w_r x_r / sum_P pi_r w_r
 * with the same start (nu = 20), bracket, root finder, stop rule and status codes; integer weights give the fit of the
 * repeated rows.  A row of weight zero is not read beyond its weight: a NaN or inf in it reaches no sum.  One
 * single-workgroup kernel ahead of the loop forms W, sum w^2, |P| and a bad-weight flag in a fixed order, and the host
 * reads that record once: a negative, NaN or inf weight, or |P| <= D, fails the call before any EM kernel is launched
 * (mu_io / sigma_io untouched).  result: HOST f64 [6] <- { nu, iterations, status, host reads = 1 + ceil(iterations / 8),
 * |P|, the Kish effective sample size W^2 / sum w^2 }.  Fixed-order sums, no atomics: the same bits on every call.
 * 1 <= D <= PMC_STUDENT_W_MAX_D; above PMC_STUDENT_MAX_D the row pass takes 32 rows per workgroup instead of 64 (140,672
 * bytes of LDS at D = 157), with the same arithmetic per row.  workspace: pmc_student_em_weighted_workspace_bytes(n, D). */
#define PMC_STUDENT_W_MAX_D 157
int64_t pmc_student_em_weighted_workspace_bytes(int64_t n, int32_t D);
int pmc_student_em_weighted(const double* x, const float* x32, const double* w, int64_t n, int32_t D, double* mu_io,
                            double* sigma_io, double tol, int32_t max_iter, double* result, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* The full affine map of Reparameterize(diagonal=False), scaler.py:288-292 / :308-313, on rows f64 [n][D]:
 * mode 0: out = mu + M in (M = L: _inverse_affine), mode 1: out = M (in - mu) (M = L^-1: _forward_affine).  in != out. */
int pmc_affine_rows(const double* M, const double* mu, const double* in, double* out, int64_t n, int32_t D,
                    int32_t mode, void* stream);

/* Bootstrap of the evidence estimate, Sampler._compute_evidence, sampler.py:905-911:
 * out[b] = logsumexp(logw[choice(n, n)]) - log(n) for b < B, the draws from Philox keyed by (seed, b, draw).
 * stats f64 [>= 1] on the device: stats[0] = max(logw) (pmc_logw_stats). */
int pmc_bootstrap_logz(const double* logw, int64_t n, const double* stats, int64_t B, uint64_t seed, double* out,
                       void* stream);
/* The same with the draws given: draws i64 [B][n] on the device, values in [0, n) -- np.random.choice(n, n) of
 * sampler.py:908 as the reference drew it (parity tests replay the recorded stream). */
int pmc_bootstrap_logz_replay(const double* logw, int64_t n, const double* stats, int64_t B, const int64_t* draws,
                              double* out, void* stream);

/* Sampler._resample gather, sampler.py:707-713: dst[i] = src[idx[i]] for the five arrays. */
int pmc_gather(const int64_t* idx, int64_t n_out, int32_t D, const double* u, const double* x,
               const double* logdetj, const double* logl, const double* logp, double* u_out,
               double* x_out, double* logdetj_out, double* logl_out, double* logp_out, void* stream);

/* Resampling indices from normalised weights w f64 [P]:
 * multinomial (np.random.choice(p=w), sampler.py:703: cdf.searchsorted(uniform, 'right'))
 * with uniforms f64 [n_out]; systematic (tools.py:136-186) with one offset in [0,1).
 * cdf: f64 [P] scratch. */
int pmc_resample_multinomial(const double* w, int64_t P, const double* uniforms, int64_t n_out,
                             double* cdf, int64_t* idx, void* stream);
int pmc_resample_systematic(const double* w, int64_t P, double offset, int64_t n_out, double* cdf,
                            int64_t* idx, void* stream);

/* ----------------------------------------------------------------- flow prior */

/* A finished run's flow and scaler as a normalised density on the prior's box (pocomc_amd.FlowPrior):
 *   log p(x) = flow.log_prob(u(x)) - log|dx/du|,  u = Reparameterize.forward(x),
 * as two launches around the flow's own forward call (pmc_maf_forward / pmc_maf_forward_bf16 with log_prob on u32).
 *
 * pmc_flow_prior_pre: Reparameterize.forward (scaler.py:180-202) of n rows with its log-determinant, in one launch.
 * x: f64, element (r, j) at x[r * row_stride + j * col_stride] (strides in elements, >= 0).  The loads are coalesced for
 * (row_stride, col_stride) = (D, 1) -- a C-contiguous [n][D] -- and (1, n) -- the MCMC step's column-major view; other
 * pairs are read correctly, slowly.  s->bc is not read: the forward map has no boundary conditions.
 * u32 f32 [n][D]: u for the flow; a row with inside == 0 is written as zeros (the flow never reads a NaN or an inf).
 * ldj f64 [n]: log|dx/du| = sum_j J_j (+ sum_log_sigma when s->scale), J_j the Jacobian term of the inverse map at the
 * unscaled value the forward map has just computed (no second inversion), added j = 0, 1, ..., D - 1 by one lane: a row's
 * bits depend on its values alone -- not on the layout, on n or on the row's place in the call.
 * inside int32 [n]: 1 iff every x_j and every u_j (as float32) is finite and every bounded x_j lies strictly inside its
 * bounds.
 * Width limit: D <= 157 (the widest MCMC step; a block keeps 64 rows of x / J and of u32 in LDS: 64 * ((D | 1) * 8 + D * 4)
 * + 256 bytes).  A wider call fails with "n_dim too large" before anything is launched or written. */
int pmc_flow_prior_pre(const pmc_scaler_t* s, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,
                       float* u32, double* ldj, int32_t* inside, void* stream);

/* logp[r] = (double)lp32[r] - ldj[r] where inside[r] and that value is finite, -inf everywhere else: never NaN, never
 * +inf.  lp32 f32 [n] (the flow's log_prob of u32), ldj f64 [n], inside int32 [n], logp f64 [n]. */
int pmc_flow_prior_post(const float* lp32, const double* ldj, const int32_t* inside, double* logp, int64_t n,
                        void* stream);

/* ----------------------------------------------------------------- joint prior */

/* A flow prior on Df columns of x and a table of scipy factors on the other Dr (pocomc_amd.JointPrior), D = Df + Dr:
 *   log p(x) = [flow.log_prob(u(x_F)) - log|dx_F/du|] + sum_m dist_m.logpdf(x[rest_cols[m]]),  u = Reparameterize.forward(x_F),
 *   x_F[k] = x[flow_cols[k]],
 * as two launches around the flow's own forward call, like the flow prior's.
 *
 * pmc_joint_prior_pre: pmc_flow_prior_pre on the flow block's columns and pmc_prior_logpdf on the others, in ONE launch that
 * reads the tile of x once.  s: the flow block's scaler (s->D = Df features; s->bc is not read).  rest: the table of the
 * other factors (rest->D = Dr).  flow_cols int32 [Df], rest_cols int32 [Dr], device memory: the column of x that is flow
 * feature k / rest factor m; together a permutation of 0 .. D - 1.  The entry does not read them (device memory: the caller
 * checks their content, JointPrior.layout); the kernel does not follow an entry outside [0, D): every row of the call's
 * blocks then gets inside = 0.
 * x: f64, element (r, j) at x[r * row_stride + j * col_stride], j < D, with the two coalesced layouts (D, 1) and (1, n) of
 * pmc_flow_prior_pre; other strides are read correctly, slowly.
 * u32 f32 [n][Df], ldj f64 [n]: what pmc_flow_prior_pre writes for the gathered C-contiguous flow columns, bit for bit
 * (the same element routine, the Jacobian terms added k = 0, 1, ..., Df - 1 by one lane).
 * rest_logp f64 [n]: lp = 0.0; lp += term_m, m = 0, 1, ..., Dr - 1 -- the bits of pmc_prior_logpdf on the gathered rest
 * columns.  Outside a factor's support its term, and so the sum, is -inf; at a pole of a family the sum may be +inf
 * (pmc_joint_prior_post maps it).
 * inside int32 [n]: 1 iff every x_j of the row (flow and rest) is finite, every flow column passes pmc_flow_prior_pre's test
 * (strictly inside the scaler's bounds, a finite float32 u) and no rest term is NaN.  A rest factor's own support is not
 * part of it.  A row with inside == 0 is written as zeros to u32 and as -inf to rest_logp.
 * A row's bits depend on its values alone -- not on the layout, on n or on the row's place in the call.
 * Refused before anything is launched or written, each with a text of its own: a NULL pointer or a negative count or
 * stride; Df < 2; Dr < 1; Df + Dr > 157 ("n_dim too large"; a block keeps 64 rows of x and of u32 in LDS:
 * 64 * ((D | 1) * 8 + Df * 4) + 256 + 4 D bytes); rest->n_extended > 0 without rest->par; s->scale without mu / sigma; more
 * than 2^31 - 1 blocks of 64 rows.  n == 0 returns 0. */
int pmc_joint_prior_pre(const pmc_scaler_t* s, const int32_t* flow_cols, const pmc_prior_t* rest, const int32_t* rest_cols,
                        const double* x, int64_t row_stride, int64_t col_stride, int64_t n, float* u32, double* ldj,
                        double* rest_logp, int32_t* inside, void* stream);

/* v = ((double)lp32[r] - ldj[r]) + rest_logp[r], in this order; logp[r] = v where inside[r] and v is finite, -inf everywhere
 * else: never NaN, never +inf (a pole of a table family, such as gamma(a < 1) at its loc, is -inf).  lp32 f32 [n] (the
 * flow's log_prob of u32), ldj, rest_logp f64 [n], inside int32 [n], logp f64 [n]. */
int pmc_joint_prior_post(const float* lp32, const double* ldj, const double* rest_logp, const int32_t* inside, double* logp,
                         int64_t n, void* stream);

/* ----------------------------------------------------------------- joint prior, several flow blocks */

/* B flow priors on disjoint blocks of columns and an optional table on the others (pocomc_amd.JointPrior, the blocks form),
 * D = sum_b Df_b + Dr:
 *   log p(x) = sum_b [flow_b.log_prob(u_b(x_{F_b})) - log|dx_{F_b}/du_b|] + sum_m dist_m.logpdf(x[rest_cols[m]]),
 * as B + 2 launches and one pass over x: pmc_joint_blocks_pre, every block's own forward call on its piece of u32 (in block
 * order), pmc_joint_blocks_post.  Appended within ABI 9: new entries and a new struct only.
 *
 * scaler[b]: block b's scaler, a host struct that points to device arrays (scaler[b]->D = Df_b >= 2; bc is not read); the
 * blocks may differ in transform (logit) and in the affine part (scale).  cols[b]: int32 [Df_b], device memory: the column of
 * x that is block b's feature k.  rest / rest_cols: the table and its columns (int32 [Dr], device memory) as for
 * pmc_joint_prior_pre, or both NULL: no table, Dr = 0.  All maps together are a permutation of 0 .. D - 1 (the caller's to
 * check: JointPrior.layout_blocks); an entry outside [0, D) is not followed, every row of the call's blocks then gets
 * inside = 0.  Entries b >= n_blocks are not read.
 * D: the columns of x where the maps do not cover them all (the other columns belong to correlated normal blocks, see
 * pmc_gauss_blocks_t): sum_b Df_b + Dr <= D <= 157; the maps are then distinct entries of [0, D), the tile holds D columns
 * and the bits of every output are those of the call on the gathered columns.  D = 0 is what every caller passed so far:
 * the maps are a permutation.  The stage of a step (pmc_prior_blocks_stage_t) takes D = 0, or the step's D with maps that
 * cover it. */
#define PMC_JOINT_BLOCKS_MAX 8
typedef struct pmc_joint_blocks {
    int32_t n_blocks;             /* 1 .. PMC_JOINT_BLOCKS_MAX */
    int32_t D;                    /* columns of x; 0 (the field was reserved): sum_b Df_b + Dr */
    const pmc_scaler_t* scaler[PMC_JOINT_BLOCKS_MAX];
    const int32_t* cols[PMC_JOINT_BLOCKS_MAX];
    const pmc_prior_t* rest;      /* or NULL */
    const int32_t* rest_cols;     /* or NULL (with rest) */
} pmc_joint_blocks_t;

/* One launch with pmc_joint_prior_pre's shape and stride contract (64 rows of all D columns through LDS, the two coalesced
 * layouts (D, 1) and (1, n), one thread per slot, one lane per row for the sums).  The slots: block 0's features, block
 * 1's, ..., then the rest factors.
 * u32 f32: block b's [n][Df_b] array starts n * (Df_0 + ... + Df_{b-1}) floats into u32 (sum_b n * Df_b floats in all).
 * ldj f64 [B][n].  rest_logp f64 [n]: not written, and may be NULL, without a table.  inside int32 [n]: ONE flag per row:
 * every x_j finite, every block's columns pass pmc_flow_prior_pre's test, no rest term NaN.
 * On every row with inside == 1, block b's piece of u32 and ldj[b] are what pmc_flow_prior_pre writes for the gathered
 * C-contiguous block, and rest_logp what pmc_prior_logpdf gives on the gathered rest, bit for bit.  A row with inside == 0
 * is zeros in every block's u32 and -inf in rest_logp.  A row's bits depend on its values alone.
 * Refused before anything is launched or written, each with a text of its own: a NULL descriptor or NULL fields; n_blocks
 * outside 1 .. 8; a block with Df_b < 2; sum Df_b + Dr > 157 ("n_dim too large"; LDS as for pmc_joint_prior_pre with Df the
 * blocks' sum, 64 * (D | 1) * 8 for the tile with D set); D set and smaller than sum Df_b + Dr, or larger than 157;
 * rest->n_extended > 0 without rest->par; a scaler with scale and no mu / sigma; a NULL array, a negative
 * count or stride; more than 2^31 - 1 blocks of 64 rows.  n == 0 returns 0 and reads no array. */
int pmc_joint_blocks_pre(const pmc_joint_blocks_t* j, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,
                         float* u32, double* ldj, double* rest_logp, int32_t* inside, void* stream);

/* v = (double)lp32[0][r] - ldj[0][r]; v = v + ((double)lp32[b][r] - ldj[b][r]) for b = 1 .. n_blocks - 1; with rest_logp
 * non-NULL v = v + rest_logp[r]; logp[r] = v where inside[r] and v is finite, -inf everywhere else: never NaN, never +inf.
 * lp32 f32 [n_blocks][n] (block b's log_prob of its piece of u32), ldj f64 [n_blocks][n], rest_logp f64 [n] or NULL.  One
 * block: pmc_joint_prior_post's bits with a table, pmc_flow_prior_post's without. */
int pmc_joint_blocks_post(int32_t n_blocks, const float* lp32, const double* ldj, const double* rest_logp,
                          const int32_t* inside, double* logp, int64_t n, void* stream);

/* The blocks form inside the step of a HOST likelihood: what pmc_prior_stage_t is for one flow block, for several.  The
 * descriptor of pmc_joint_blocks_pre by value, every block's flow (maf[b]; precision="bf16": its image and per_t, else NULL
 * and 0) and the workspaces for the n rows of one pmc_step_t: u32 and ldj laid out as pmc_joint_blocks_pre writes them,
 * lp32 f32 [n_blocks][n], ONE z of n * max_b Df_b floats (the flows run one after another on the stream and nobody reads
 * z), rest_logp f64 [n] (NULL without a table), inside int32 [n]; count / h_count: pmc_prior_stage_t's count protocol,
 * unchanged.  Entries b >= blocks.n_blocks are not read. */
typedef struct pmc_prior_blocks_stage {
    pmc_joint_blocks_t blocks;
    const pmc_maf_t* maf[PMC_JOINT_BLOCKS_MAX];
    const uint16_t* image16[PMC_JOINT_BLOCKS_MAX];
    int64_t image_per_transform[PMC_JOINT_BLOCKS_MAX];
    float* u32;
    float* z;
    float* lp32;
    double* ldj;
    double* rest_logp;
    int32_t* inside;
    unsigned long long* count;
    int64_t* h_count;
} pmc_prior_blocks_stage_t;

/* pmc_step_ext_t with one more field behind it, announced by step.ext = PMC_STEP_EXT2 (callers with ext = 0 or
 * ext = PMC_STEP_EXT read exactly what they read before: nothing behind the struct they allocated).  At most one of the
 * two pointers is non-NULL; with both set every call that would place the stage refuses it.  blocks_stage stands where
 * prior_stage stands: pmc_step_prior_stage, pmc_step_pre and the pipeline enqueue it behind the hand-over (the pipeline:
 * behind the LAST lane's pre-step, in front of the fills) as pmc_joint_blocks_pre on p_x, the blocks' forward calls in
 * block order and a closing kernel that writes p_logp -- pmc_joint_blocks_post's join where p_fin != 0, -inf elsewhere --
 * and counts the rows with p_fin != 0 and no finite logp' into h_count[launch & 1]; pmc_step_post takes logp' from p_logp.
 * The stage check refuses, before any launch: NULL workspaces, a block without its scaler or flow, a width that is not
 * the step's D, a flow whose width is not its scaler's, both pointers set, and what pmc_joint_blocks_pre refuses, in its
 * words. */
#define PMC_STEP_EXT2 2
typedef struct pmc_step_ext2 {
    pmc_step_t step;
    const pmc_prior_stage_t* prior_stage;
    const pmc_prior_blocks_stage_t* blocks_stage;
} pmc_step_ext2_t;

/* ----------------------------------------------------------------- correlated normal blocks */

/* B correlated normal blocks on disjoint blocks of columns of x (pocomc_amd.GaussianPrior; the Gaussian blocks of
 * pocomc_amd.JointPrior), on top of a value that is already there (base), of a table of scipy factors (rest) or of nothing:
 *   log p(x) = start + sum_b g_b,   g_b = -0.5 |Linv_b (x[cols_b] - mean_b)|^2 - logc_b,
 * Linv_b the inverse of the lower Cholesky factor of block b's covariance and logc_b = sum log diag(L_b) + dim_b / 2
 * log(2 pi), both from the host in float64.  ONE launch, float64, one pass over x.  Appended within ABI 9: a new entry and
 * a new struct only.
 *
 * dim[b] >= 1 columns per block; cols[b] int32 [dim[b]], mean[b] f64 [dim[b]], linv[b] f64 [dim[b] (dim[b] + 1) / 2]: row i
 * of Linv_b holds its i + 1 entries at i (i + 1) / 2; all device memory.  D: the columns of x (the blocks and the rest need
 * not cover them all).  rest / rest_cols: a table and its columns (int32 [rest->D], device memory) as for
 * pmc_joint_blocks_pre, or both NULL.  The maps are the caller's to check (JointPrior.layout_blocks): distinct entries of
 * [0, D); an entry outside [0, D) is not followed, every row of its launch block of 64 rows then gets -inf.  Entries
 * b >= n_blocks are not read.
 *
 * The arithmetic, every product and every sum rounded to float64 (no FMA), for a row and a block:
 *   d_j = x[cols[j]] - mean[j]
 *   y_i = (((0.0 + Linv[i,0] d_0) + Linv[i,1] d_1) + ...) + Linv[i,i] d_i
 *   q   = ((0.0 + y_0 y_0) + y_1 y_1) + ...                   in i order
 *   g   = -0.5 q - logc
 * logp[r] = v = start + g_0 + g_1 + ..., left to right; start = base[r] with base (f64 [n]; may be logp itself: in place),
 * else lp = 0.0; lp += term_m, m = 0 .. rest->D - 1 with rest (the bits of pmc_prior_logpdf on the gathered rest columns),
 * else nothing: v = g_0 (+ g_1 ...).  -inf where an x_j of a block or rest column is not finite, a rest term is NaN or v is
 * not finite (a NaN of the arithmetic, a pole of a table family): never NaN, never +inf.
 * x: f64, element (r, j) at x[r * row_stride + j * col_stride], with the two coalesced layouts (D, 1) and (1, n) of
 * pmc_flow_prior_pre; other strides are read correctly, slowly.  A row's bits depend on its values alone -- not on the
 * layout, on n or on the row's place in the call.
 * Refused before anything is launched or written, each with a text of its own: a NULL descriptor or NULL block arrays;
 * n_blocks outside 1 .. 8; a block with dim < 1; D > 157 ("n_dim too large"; a launch block keeps 64 rows of x in LDS:
 * 64 * (D | 1) * 8 + 256 bytes); more block and rest columns than D; rest without rest_cols or the reverse;
 * rest->n_extended > 0 without rest->par; base and rest together; a NULL x or logp, a negative count or stride; more than
 * 2^31 - 1 blocks of 64 rows.  n == 0 returns 0 and reads no array. */
#define PMC_GAUSS_BLOCKS_MAX 8
typedef struct pmc_gauss_blocks {
    int32_t n_blocks;             /* 1 .. PMC_GAUSS_BLOCKS_MAX */
    int32_t D;                    /* columns of x */
    int32_t dim[PMC_GAUSS_BLOCKS_MAX];
    const int32_t* cols[PMC_GAUSS_BLOCKS_MAX];
    const double* mean[PMC_GAUSS_BLOCKS_MAX];
    const double* linv[PMC_GAUSS_BLOCKS_MAX];
    double logc[PMC_GAUSS_BLOCKS_MAX];
    const pmc_prior_t* rest;      /* or NULL */
    const int32_t* rest_cols;     /* or NULL (with rest) */
} pmc_gauss_blocks_t;

int pmc_gauss_blocks_logpdf(const pmc_gauss_blocks_t* g, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,
                            const double* base, double* logp, void* stream);

/* The same blocks, some of them restricted to a closed box (pocomc_amd.TruncatedGaussianPrior, alone or as a block of
 * pocomc_amd.JointPrior): pmc_gauss_blocks_logpdf's contract plus one rule -- a row with any x[cols_b[j]] that is not in
 * [lo_b[j], hi_b[j]] gets -inf.  The test is !(x >= lo && x <= hi): the value on a bound is finite, the first float beyond
 * it is -inf, and a NaN fails it.  Every other row has exactly the bits pmc_gauss_blocks_logpdf gives for the same
 * descriptor; the caller puts logc + log_mass, the log of the box's mass under the block's normal, into g->logc[b].
 * Appended within ABI 9: a new entry and a new struct only; the kernel is a second instance of the same template, the
 * entry above launches the instance without the test.
 * Refused before anything is launched or written: everything pmc_gauss_blocks_logpdf refuses, with the same texts under
 * this entry's name; a NULL box; a block with one of lo / hi set and the other NULL.  Entries b >= n_blocks are not read.
 * n == 0 returns 0 and reads no array. */
typedef struct pmc_gauss_box {            /* per block of the pmc_gauss_blocks_t it goes with */
    const double* lo[PMC_GAUSS_BLOCKS_MAX];   /* f64 [dim[b]], device memory, -inf allowed; NULL with hi[b]: block b has no box */
    const double* hi[PMC_GAUSS_BLOCKS_MAX];
} pmc_gauss_box_t;
int pmc_gauss_box_logpdf(const pmc_gauss_blocks_t* g, const pmc_gauss_box_t* box, const double* x, int64_t row_stride,
                         int64_t col_stride, int64_t n, const double* base, double* logp, void* stream);

/* ----------------------------------------------------------------- a mixture of correlated normals */

/* A mixture of C correlated normals on one block of dim columns of x (pocomc_amd.GaussianMixturePrior; the mixture blocks
 * of pocomc_amd.JointPrior), on top of a value that is already there (base), of a table of scipy factors (rest) or of
 * nothing:
 *   log p(x) = start + log sum_c w_c N(x[cols]; mean_c, cov_c).
 * ONE launch, float64, one pass over x.  Appended within ABI 9: a new entry and a new struct only.
 *
 * 1 <= n_comp <= 32 components (PMC_GAUSS_MIX_MAX_COMPONENTS) on the same 1 <= dim <= 64 columns (PMC_GAUSS_MIX_MAX_DIM);
 * cols int32 [dim]; logw f64 [C], the logs of the normalised weights; mean f64 [C][dim]; linv f64 [C][dim (dim + 1) / 2], each
 * component's inverse Cholesky factor packed by rows as in pmc_gauss_blocks_t; logc f64 [C] (its formula there); all device
 * memory.  D: the columns of x.  rest / rest_cols: a table and its columns as in pmc_gauss_blocks_t, or both NULL.  The map
 * is the caller's to check: distinct entries of [0, D); an entry outside [0, D) is not followed, every row of its launch
 * block of 64 rows then gets -inf.
 *
 * The arithmetic of a row, every product and every sum rounded to float64 (no FMA):
 *   g_c = pmc_gauss_blocks_logpdf's g for (mean_c, Linv_c, logc_c): d_j, y_i, q in i order, g = -0.5 q - logc_c
 *   t_c = g_c + logw_c                          (-inf where g_c is NaN or -inf)
 *   m   = max_c t_c
 *   s   = ((0.0 + exp(t_0 - m)) + exp(t_1 - m)) + ...      in c order
 *   v   = m + log(s);   logp[r] = start + v
 * start = base[r] with base (f64 [n]; may be logp itself: in place), else lp = 0.0; lp += term_m, m = 0 .. rest->D - 1 with
 * rest (the bits of pmc_prior_logpdf on the gathered rest columns), else nothing: logp[r] = v.  base and rest exclude each
 * other.  The t_c are the bits of the numpy statement (tests/gauss_mix_model.py); exp and log are the device library's, so
 * v lies within (C + 8) 2^-52 + 2^-52 |v| of that statement's.  With one component and logw_0 = 0.0 the value has
 * pmc_gauss_blocks_logpdf's bits (exp(0) = 1, log(1) = 0).
 * -inf where an x_j of a block or rest column is not finite, a rest term is NaN, every t_c is -inf (m = -inf: the
 * differences are never formed) or the result is not finite: never NaN, never +inf.
 * x: f64, element (r, j) at x[r * row_stride + j * col_stride], with the two coalesced layouts (D, 1) and (1, n); other
 * strides are read correctly, slowly.  A row's bits depend on its values alone -- not on the layout, on n or on the row's
 * place in the call.
 * Refused before anything is launched or written, each with a text of its own: a NULL descriptor; a NULL array inside it;
 * n_comp outside 1 .. 32; dim outside 1 .. 64; D > 157 ("n_dim too large"; a launch block keeps 64 rows of x, a work tile
 * and every component's t in LDS: 64 * ((D | 1) + (dim | 1) + n_comp) * 8 + 256 bytes, 130304 at the three limits, under
 * the 163840 of a workgroup); dim + rest->D > D; rest without rest_cols or the reverse; a rest without its arrays;
 * rest->n_extended > 0 without rest->par; base and rest together; a NULL x or logp; a negative count or stride; more than
 * 2^31 - 1 blocks of 64 rows.  n == 0 returns 0 and reads no array. */
#define PMC_GAUSS_MIX_MAX_COMPONENTS 32
#define PMC_GAUSS_MIX_MAX_DIM 64
typedef struct pmc_gauss_mix {
    int32_t n_comp;               /* 1 .. PMC_GAUSS_MIX_MAX_COMPONENTS */
    int32_t dim;                  /* 1 .. PMC_GAUSS_MIX_MAX_DIM */
    int32_t D;                    /* columns of x */
    int32_t reserved;             /* 0 */
    const int32_t* cols;          /* [dim] */
    const double* logw;           /* [n_comp] */
    const double* mean;           /* [n_comp][dim] */
    const double* linv;           /* [n_comp][dim (dim + 1) / 2] */
    const double* logc;           /* [n_comp] */
    const pmc_prior_t* rest;      /* or NULL */
    const int32_t* rest_cols;     /* or NULL (with rest) */
} pmc_gauss_mix_t;

int pmc_gauss_mix_logpdf(const pmc_gauss_mix_t* g, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,
                         const double* base, double* logp, void* stream);

/* ----------------------------------------------------------------- a weighted Gaussian KDE of samples */

/* A kernel density estimate of M weighted samples with one shared bandwidth matrix H on one block of dim columns of x
 * (pocomc_amd.KDEPrior; the KDE blocks of pocomc_amd.JointPrior), on top of a value that is already there (base), of a
 * table of scipy factors (rest) or of nothing:
 *   log p(x) = start + log sum_m w_m N(x[cols]; s_m, H).
 * ONE launch, float64, one pass over x.  Appended within ABI 9: a new entry and a new struct only.
 *
 * 1 <= n_samples <= 65536 samples (PMC_KDE_MAX_SAMPLES) on 1 <= dim <= 16 columns (PMC_KDE_MAX_DIM); cols int32 [dim];
 * center f64 [dim], the weighted mean of the samples; linv f64 [dim (dim + 1) / 2], the inverse of H's lower Cholesky factor
 * packed by rows as in pmc_gauss_blocks_t; t f64 [n_samples][dim], the whitened samples t_m = Linv (s_m - center); logw f64
 * [n_samples], the logs of the normalised weights; all device memory.  logc = dim / 2 log(2 pi) + 1/2 log|H|, by value.
 * D: the columns of x.  rest / rest_cols: a table and its columns as in pmc_gauss_blocks_t, or both NULL.  The map is the
 * caller's to check: distinct entries of [0, D); an entry outside [0, D) is not followed, every row of its launch block of
 * 64 rows then gets -inf.
 *
 * The statement of a row (tests/kde_model.py), every product and every sum rounded to float64 (no FMA):
 *   d_j = x[cols[j]] - center_j
 *   y_i = (((0.0 + Linv[i,0] d_0) + Linv[i,1] d_1) + ...) + Linv[i,i] d_i          (pmc_gauss_blocks_logpdf's y)
 *   q_m = ((0.0 + (y_0 - t_m0)^2) + (y_1 - t_m1)^2) + ...                         in j order
 *   e_m = -0.5 q_m + logw_m
 *   mx  = max_m e_m                              (-inf: the row is -inf)
 *   s   = sum_m exp(e_m - mx)
 *   v   = (mx + log(s)) - logc;   logp[r] = start + v
 * start = base[r] with base (f64 [n]; may be logp itself: in place), else lp = 0.0; lp += term_m, m = 0 .. rest->D - 1 with
 * rest (the bits of pmc_prior_logpdf on the gathered rest columns), else nothing: logp[r] = v.  base and rest exclude each
 * other.  The y_i and every e_m have the statement's bits.  The kernel cuts the samples in eight contiguous slices of
 * ceil(M / 8) -- a cut that depends on M alone -- adds each slice's exps in m order and the eight partial sums in slice
 * order; exp and log are the device library's.  v lies within (M + 8) 2^-52 + 2^-50 (|v| + |logc|) of the statement
 * evaluated with a sequential sum.  With one sample and logw_0 = 0.0 the value has pmc_gauss_blocks_logpdf's bits for
 * (mean = s_0, H): t_0 = 0, exp(0) = 1, log(1) = 0.
 * -inf where an x_j of a block or rest column is not finite, a rest term is NaN, every e_m is -inf or NaN (mx = -inf) or
 * the result is not finite: never NaN, never +inf.
 * x: f64, element (r, j) at x[r * row_stride + j * col_stride], with the two coalesced layouts (D, 1) and (1, n); other
 * strides are read correctly, slowly.  A row's bits depend on its values and the descriptor alone -- not on the layout, on
 * n or on the row's place in the call.
 * Refused before anything is launched or written, each with a text of its own: a NULL descriptor; a NULL array inside it;
 * n_samples outside 1 .. 65536; dim outside 1 .. 16; D > 157 ("n_dim too large"; a launch block keeps 64 rows of x and the
 * eight wavefronts' partial maxima and sums in LDS: 64 * ((D | 1) + 16) * 8 + 256 bytes, 88832 at D = 157); dim + rest->D
 * > D; rest without rest_cols or the reverse; a rest without its arrays; rest->n_extended > 0 without rest->par; base and
 * rest together; a NULL x or logp; a negative count or stride; more than 2^31 - 1 blocks of 64 rows.  n == 0 returns 0 and
 * reads no array. */
#define PMC_KDE_MAX_DIM 16
#define PMC_KDE_MAX_SAMPLES 65536
typedef struct pmc_kde {
    int32_t n_samples;            /* 1 .. PMC_KDE_MAX_SAMPLES */
    int32_t dim;                  /* 1 .. PMC_KDE_MAX_DIM */
    int32_t D;                    /* columns of x */
    int32_t reserved;             /* 0 */
    const int32_t* cols;          /* [dim] */
    const double* center;         /* [dim] */
    const double* linv;           /* [dim (dim + 1) / 2] */
    const double* t;              /* [n_samples][dim] */
    const double* logw;           /* [n_samples] */
    double logc;
    const pmc_prior_t* rest;      /* or NULL */
    const int32_t* rest_cols;     /* or NULL (with rest) */
} pmc_kde_t;

int pmc_kde_logpdf(const pmc_kde_t* g, const double* x, int64_t row_stride, int64_t col_stride, int64_t n,
                   const double* base, double* logp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POCOMC_AMD_H */
