// Which flow-inverse kernel runs: the one place that decides it (host code only, no kernel).
//
// Nine kernels invert a flow (pocomc/mcmc.py:88, every preconditioned step): the two D-pass kernels of the reference's
// algorithm (the workgroup one in a full and a lean instance), the register-chain sweeps of the affine flows with one (SOLO) or two (DUO) wavefronts per 16 walkers, the
// lane-per-walker sweep (LANE), the spline sweeps with one (NSF_SOLO) or two (NSF_DUO) wavefronts, the workgroup sweeps of the affine flows
// (WG) and of the spline flows (WG_NSF), both on request only.  pmc_plan_inverse maps
// (flow, rows, algo) to the instance pmc_maf_inverse / pmc_step_pre launch -- or, asked for the fused launch, to the
// proposal + inverse (+ scaler epilogue) instance of the step, if there is one.  What a sweep covers is a predicate below;
// AUTO's preferences are measured.  The measurement builds' A/B switches are read here only.
#include "inverse_lds.h"
#include "scaler_body.h"

// ---- A/B switches (make DEBUG_HOOKS=1; the product library never reads the environment)
static bool lane_switch() { static const bool on = pmc_env_int("PMC_INVERSE_LANE", 0) != 0; return on; }     // 1: AUTO takes the lane sweep wherever it covers the flow
static int duo_mode() { static const int mode = pmc_env_int("PMC_INVERSE_DUO", -1); return mode; }           // -1 automatic (by size), 0 never, 1 always
static bool nsf_duo_off() { static const int mode = pmc_env_int("PMC_INVERSE_NSF_DUO", -1); return mode == 0; }   // 0: the two-wave spline sweep covers nothing
static int lane_five_min() { static const int v = pmc_env_int("PMC_TRI6_FIVE_MIN", 16); return v; }
static int lane_forced_subsets() { static const int v = pmc_env_int("PMC_TRI6_SUBSETS", 0); return v; }

// ---- what the sweeps cover
static bool affine_tri(const pmc_maf_t* m) { return m->n_out == 2 && m->tri_ok; }
// one buffer resource per transform (32-bit offsets) / over the whole image (offsets below the out-of-range lane offset)
static bool transform_offsets_ok(const pmc_maf_t* m) { return m->pk_per_transform * 4 <= 0x7fffffffLL; }
static bool image_offsets_ok(const pmc_maf_t* m) { return m->pk_per_transform * 4 * m->T < (int64_t)OOB_VOFF; }
static int chain_maxo(const pmc_maf_t* m) { return m->nOT <= 4 ? 4 : 8; }
static int fused_fm(const pmc_maf_t* m) { return m->D <= 16 ? 4 : m->D <= 32 ? 8 : 16; }

static bool solo_covers(const pmc_maf_t* m) {
    return affine_tri(m) && m->nOT <= 8 && transform_offsets_ok(m) && pmc_lds_solo(m, chain_maxo(m)) <= PMC_LDS_CAP;
}
static bool duo_covers(const pmc_maf_t* m) {
    return affine_tri(m) && m->nOT <= 8 && m->D <= 64 && image_offsets_ok(m) && pmc_lds_duo(m, chain_maxo(m)) <= PMC_LDS_CAP;
}
// The right-looking two-wave sweep takes ~0.55 of the lone wave's time per round, and a launch beyond the 512
// resident walker sets simply runs its surplus workgroups as they find a CU: it is taken whenever its LDS fits.
static bool duo_wanted(const pmc_maf_t* m) {
    return duo_mode() >= 0 ? duo_mode() != 0 : pmc_lds_duo(m, chain_maxo(m)) <= PMC_LDS_CAP;
}
static bool wg_sweep_covers(const pmc_maf_t* m) {
    return affine_tri(m) && transform_offsets_ok(m) && pmc_lds_wg_sweep(m) <= PMC_LDS_CAP;
}
static bool wg_nsf_sweep_covers(const pmc_maf_t* m) {
    return m->n_out == 23 && m->tri_ok && transform_offsets_ok(m) && pmc_lds_wg_nsf_sweep(m) <= PMC_LDS_CAP;
}
static bool nsf_duo_covers(const pmc_maf_t* m) {
    return !nsf_duo_off() && m->n_out == 23 && m->tri_ok && m->D <= 64 && m->D >= 2 && image_offsets_ok(m) &&
           pmc_lds_nsf_duo(m) <= PMC_LDS_CAP;
}

static int lane_hb(const pmc_maf_t* m) { return (m->lane16 && (m->lane16_fmt == 1 || m->lane16_fmt == 2)) ? m->lane16_fmt : 0; }
// the five-wavefront variant: plain float32 inverse of a flow with >= 16 hidden tiles, one or two subsets (the kernel must
// stay within 256 registers: two wavefronts share a SIMD, and only one such workgroup fits a CU).  With 16-bit helper
// operands the helpers are an order of magnitude below the chain: four wavefronts, a SIMD each.
static bool lane_five(const pmc_maf_t* m, bool fused, int hb) {
    return !fused && !hb && m->nT >= lane_five_min() && !(m->reserved & PMC_MAF_VARIANT_LANE_FOUR);
}
// walker subsets per workgroup: as few as keep the launch in one round (a chain wavefront takes the same time for 16
// and for 64 walkers; the helpers' share grows with the subsets), as many as the LDS admits otherwise.  0: none fits
static int lane_subsets(const pmc_maf_t* m, int64_t n, bool fused, int hb) {
    const int forced = lane_forced_subsets();
    int best = 0;
    for (int ns = 1; ns <= (lane_five(m, fused, hb) ? 2 : 4); ns *= 2) {
        if (pmc_lds_lane(m, ns, hb) > PMC_LDS_CAP) break;
        if (forced == ns) return ns;
        best = ns;
        // one workgroup per CU: the five-wave variant by construction, the four-wave instances by their registers (264-416)
        if (!forced && (n + 16 * ns - 1) / (16 * ns) <= 256) break;
    }
    return best;
}
// hb: the helpers' operands (the caller's: PMC_INVERSE_TRIANGULAR_LANE takes float32 whatever image is attached)
static bool lane_covers(const pmc_maf_t* m, int64_t n, bool fused, int hb) {
    if (!affine_tri(m) || !transform_offsets_ok(m)) return false;
    if (fused && (m->D > 64 || hb)) return false;        // (no fused instance beyond D = 64 or with 16-bit helpers)
    if (m->nT > 64) return false;                        // (a lane per hidden tile holds its rank words)
    if (hb && m->Dp * 16 > 3 * ((m->nT + 1) >> 1) * 256) return false;   // (the in-place re-rank parks x in the activation arrays)
    return lane_subsets(m, n, fused, hb) > 0;
}
// AUTO's choice between the lane-per-walker sweep and the register-chain sweeps for the flows both cover (D <= 64): with
// >= 16 hidden tiles the five-wavefront variant is faster -- D = 50 / maf6 (25 tiles): 314 us per round of <= 4096 walkers
// against 645-650 us of the two-wave sweep for <= 8192; D = 64 / maf3 (17 tiles): 120 against 160 us -- below that the
// two-wave sweep is (D = 32 / maf3, 9 tiles: 61-64 against 66-83 us for up to 8192 rows).  The step then launches the
// proposal and the scaler on their own: round 5 built the fused instances of the lane sweep (proposal prologue up to
// D = 128, scaler / prior / x' epilogue, float32 and 16-bit helpers) and measured them -- the proposal (~90 us per wavefront
// at D = 128) and the scaler (~40 us) are latency chains that cost the same inside the sweep's launch as in their own, and
// the float32 five-wavefront instance has no registers for them: config 5 255 (fused) against 300 steps/s, 16-bit helpers
// 420 against 415.
static bool lane_preferred(const pmc_maf_t* m) {
    if (!affine_tri(m) || !transform_offsets_ok(m)) return false;
    const int hb = lane_hb(m);
    if (hb) return m->nT >= lane_five_min() && pmc_lds_lane(m, 1, hb) <= PMC_LDS_CAP;
    return lane_five(m, false, 0) && pmc_lds_lane(m, 1, 0) <= PMC_LDS_CAP;
}

// ---- the plan.  Returns the error message of a request that cannot be served, or NULL
static void set_plain(pmc_inverse_plan_t* p, int sweep, size_t lds) { p->sweep = sweep; p->lds_bytes = (int32_t)lds; }
static void set_chain(pmc_inverse_plan_t* p, int sweep, const pmc_maf_t* m, bool fused) {
    p->maxo = chain_maxo(m);
    p->fm = fused ? fused_fm(m) : 0;
    set_plain(p, sweep, sweep == PMC_SWEEP_DUO ? pmc_lds_duo(m, p->maxo) : pmc_lds_solo(m, p->maxo));
}
static void set_lane(pmc_inverse_plan_t* p, const pmc_maf_t* m, int64_t n, bool fused, int hb) {
    p->subsets = lane_subsets(m, n, fused, hb);
    // wide flows (helpers saturated: their work grows with the hidden tiles, the chain's does not) get a fifth wavefront
    // for the layer-0 partials
    p->waves = (lane_five(m, fused, hb) && p->subsets <= 2) ? 5 : 4;
    p->helper_fmt = hb;
    p->fm = fused ? fused_fm(m) : 0;
    set_plain(p, PMC_SWEEP_LANE, pmc_lds_lane(m, p->subsets, hb));
}
// The lean D-pass workgroup kernel as the last resort covers the default-width flows: MAFSpec(D) has at most 51 hidden
// tiles for D <= 157, the widest MCMC step (H = 512 padded to whole quads per degree: Hp = 816 at D = 102 - 104).  Layouts
// beyond that are hand-made ones, and they keep the refusals they always had (tests/test_inverse_plan_cpu.py pins 64 and
// 65 tiles at D = 66 to the D-pass kernel's error): D + 1 full passes of a wider flow are not a plan to fall into silently.
#define PMC_LEAN_DPASS_MAX_TILES 51
static bool lean_forced(const pmc_maf_t* m) { return (m->reserved & PMC_MAF_VARIANT_LEAN_LDS) != 0; }
static bool set_dpass_lean(pmc_inverse_plan_t* p, const pmc_maf_t* m) {
    const size_t lds = pmc_lds_wg(m, 8, pmc_wg_panel_tiles(m), 1, 1);
    if (lds > PMC_LDS_CAP || (!lean_forced(m) && m->nT > PMC_LEAN_DPASS_MAX_TILES)) return false;
    set_plain(p, PMC_SWEEP_DPASS_LEAN, lds);
    return true;
}
static const char* set_dpass(pmc_inverse_plan_t* p, const pmc_maf_t* m) {
    const bool affine = m->n_out == 2;
    const size_t lds = affine ? pmc_lds_dense(m, 3) : pmc_lds_wg(m, 8, m->n_out, 1);
    if (lean_forced(m) || lds > PMC_LDS_CAP) {
        if (set_dpass_lean(p, m)) return nullptr;
        return affine ? "MAF too wide for one wave's LDS budget (160 KiB)" : "pmc_maf_forward: flow too wide for 160 KB of LDS";
    }
    set_plain(p, affine ? PMC_SWEEP_DPASS_AFFINE : PMC_SWEEP_DPASS_SPLINE, lds);
    return nullptr;
}

// the fused proposal + inverse instance of the step (AUTO / TRIANGULAR), if there is one; any: also for the flows AUTO
// gives to the lane-per-walker sweep (pmc_propose_inverse names the fused launch itself)
static void plan_fused(const pmc_maf_t* m, int64_t n, int algo, bool any, bool want_epilogue, int scaler_D, pmc_inverse_plan_t* p) {
    if (algo != PMC_INVERSE_AUTO && algo != PMC_INVERSE_TRIANGULAR) return;
    // the scaler as the sweep's epilogue: its scratch aliases the activation arrays of the walker set
    const bool epi = want_epilogue && scaler_D == m->D;
    if (m->n_out == 23) {                                // spline flows: the two-wave spline sweep has the fused instances
        if (!nsf_duo_covers(m)) return;
        set_plain(p, PMC_SWEEP_NSF_DUO, pmc_lds_nsf_duo(m));
        p->fm = fused_fm(m);
        p->epilogue = epi && scaler_epilogue_lds_bytes(m->D) <= (size_t)3 * m->Hp * 16 * sizeof(float);
    } else {
        // affine flows, D <= 64, not those AUTO gives to the lane-per-walker sweep: they take the proposal and the scaler as
        // launches of their own (lane_preferred)
        if (!solo_covers(m) || m->D > 64 || (!any && lane_preferred(m))) return;
        p->epilogue = epi && !lane_switch() && scaler_epilogue_lds_bytes(m->D) <= (size_t)2 * m->Hp * 16 * sizeof(float);
        if (lane_switch() && lane_covers(m, n, true, lane_hb(m))) set_lane(p, m, n, true, 0);
        else set_chain(p, (duo_wanted(m) && duo_covers(m)) ? PMC_SWEEP_DUO : PMC_SWEEP_SOLO, m, true);
    }
    p->fused = 1;
}

static const char* plan_spline(const pmc_maf_t* m, int algo, pmc_inverse_plan_t* p) {
    // triangular sweep, or the D-pass algorithm of the reference (zuko) as cross-check and for layouts whose degree groups
    // exceed a tile (the sweeps are built for the reference's 8 bins; other bin counts take zuko's own D-pass algorithm)
    const bool any = algo == PMC_INVERSE_AUTO;
    if (any) algo = (m->tri_ok && m->n_out == 23) ? PMC_INVERSE_TRIANGULAR : PMC_INVERSE_NAIVE;
    if (algo == PMC_INVERSE_NAIVE) return set_dpass(p, m);
    if (algo == PMC_INVERSE_TRIANGULAR_WG_NSF) {          // (an opt-in: AUTO never comes here)
        if (!m->tri_ok) return "pmc_maf_inverse: triangular sweep needs degree groups <= one tile";
        if (m->n_out != 23) return "pmc_maf_inverse: the spline sweeps are built for 8 bins (PMC_INVERSE_NAIVE covers the others)";
        if (!wg_nsf_sweep_covers(m)) return "pmc_maf_inverse: the workgroup spline sweep needs its arrays in 160 KiB of LDS";
        set_plain(p, PMC_SWEEP_WG_NSF, pmc_lds_wg_nsf_sweep(m));
        return nullptr;
    }
    if (algo != PMC_INVERSE_TRIANGULAR && algo != PMC_INVERSE_TRIANGULAR_SOLO && algo != PMC_INVERSE_TRIANGULAR_DUO)
        return "pmc_maf_inverse: spline flows know PMC_INVERSE_TRIANGULAR (_SOLO, _DUO) and PMC_INVERSE_NAIVE";
    if (!m->tri_ok) return "pmc_maf_inverse: triangular sweep needs degree groups <= one tile";
    if (m->n_out != 23) return "pmc_maf_inverse: the spline sweeps are built for 8 bins (PMC_INVERSE_NAIVE covers the others)";
    // two wavefronts per 16 rows (D <= 64), else / on request the lone-wave sweep
    if (algo != PMC_INVERSE_TRIANGULAR_SOLO && nsf_duo_covers(m)) { set_plain(p, PMC_SWEEP_NSF_DUO, pmc_lds_nsf_duo(m)); return nullptr; }
    if (algo == PMC_INVERSE_TRIANGULAR_DUO) return "pmc_maf_inverse: the two-wave spline sweep needs D <= 64 and its tiles in 160 KiB of LDS";
    if (pmc_lds_nsf_solo(m) > PMC_LDS_CAP) {
        // (AUTO: the lean D-pass kernel covers what is left -- the full one is larger than the lone-wave sweep)
        if (any && set_dpass_lean(p, m)) return nullptr;
        return "pmc_maf_inverse: flow too wide for one wave's LDS budget (160 KiB)";
    }
    set_plain(p, PMC_SWEEP_NSF_SOLO, pmc_lds_nsf_solo(m));
    return nullptr;
}

static const char* plan_affine(const pmc_maf_t* m, int64_t n, int algo, pmc_inverse_plan_t* p) {
    const bool any = algo == PMC_INVERSE_AUTO;
    if (any) algo = m->tri_ok ? PMC_INVERSE_TRIANGULAR : PMC_INVERSE_NAIVE;
    switch (algo) {
    case PMC_INVERSE_TRIANGULAR: {
        if (!m->tri_ok) return "pmc_maf_inverse: triangular sweep needs degree groups <= one tile";
        // register-chain sweeps for flows of < 16 hidden tiles and D <= 64, the lane-per-walker sweep for the wider ones
        const int hb = lane_hb(m);
        const bool lane = lane_covers(m, n, false, hb);
        if ((lane_switch() || lane_preferred(m)) && lane) set_lane(p, m, n, false, hb);
        else if (duo_wanted(m) && duo_covers(m)) set_chain(p, PMC_SWEEP_DUO, m, false);
        else if (solo_covers(m)) set_chain(p, PMC_SWEEP_SOLO, m, false);
        else if (lane) set_lane(p, m, n, false, hb);
        else if (any) return set_dpass(p, m);            // (AUTO: the D-pass algorithm covers what is left)
        else return "pmc_maf_inverse: the triangular sweeps need their tiles in 160 KiB of LDS";
        return nullptr;
    }
    case PMC_INVERSE_TRIANGULAR_SOLO:
    case PMC_INVERSE_TRIANGULAR_DUO:
        if (!m->tri_ok) return "pmc_maf_inverse: triangular sweep needs degree groups <= one tile";
        if (algo == PMC_INVERSE_TRIANGULAR_DUO ? !duo_covers(m) : !solo_covers(m))
            return "pmc_maf_inverse: this sweep needs D <= 64 and its tiles in 160 KiB of LDS";
        set_chain(p, algo == PMC_INVERSE_TRIANGULAR_DUO ? PMC_SWEEP_DUO : PMC_SWEEP_SOLO, m, false);
        return nullptr;
    case PMC_INVERSE_TRIANGULAR_LANE:                    // (the float32 helpers, whatever is attached)
    case PMC_INVERSE_TRIANGULAR_LANE16: {
        const int hb = algo == PMC_INVERSE_TRIANGULAR_LANE16 ? lane_hb(m) : 0;
        if (algo == PMC_INVERSE_TRIANGULAR_LANE16 && !hb)
            return "pmc_maf_inverse: PMC_INVERSE_TRIANGULAR_LANE16 needs pmc_maf_t.lane16 (pmc_maf_pack_lane16)";
        if (!lane_covers(m, n, false, hb))
            return "pmc_maf_inverse: the lane-per-walker sweep needs an affine flow whose degree groups fit a tile";
        set_lane(p, m, n, false, hb);
        return nullptr;
    }
    case PMC_INVERSE_TRIANGULAR_WG:                      // (an opt-in: AUTO never comes here)
        if (!m->tri_ok) return "pmc_maf_inverse: triangular sweep needs degree groups <= one tile";
        if (!wg_sweep_covers(m)) return "pmc_maf_inverse: the workgroup sweep needs its arrays in 160 KiB of LDS";
        set_plain(p, PMC_SWEEP_WG, pmc_lds_wg_sweep(m));
        return nullptr;
    case PMC_INVERSE_NAIVE: return set_dpass(p, m);
    default: return "pmc_maf_inverse: unknown algo";
    }
}

static const char* plan_inverse(const pmc_maf_t* m, int64_t n, int algo, int fused, int want_epilogue, int scaler_D, pmc_inverse_plan_t* p) {
    *p = pmc_inverse_plan_t{};
    if (fused) { plan_fused(m, n, algo, fused == PMC_FUSED_ANY, want_epilogue != 0, scaler_D, p); return nullptr; }
    return m->n_out != 2 ? plan_spline(m, algo, p) : plan_affine(m, n, algo, p);
}

int pmc_plan_inverse(const pmc_maf_t* m, int64_t n, int algo, int fused, int want_epilogue, int scaler_D, pmc_inverse_plan_t* out) {
    const char* err = plan_inverse(m, n, algo, fused, want_epilogue, scaler_D, out);
    return err ? pmc_fail(err) : 0;
}

extern "C" int pmc_maf_inverse_plan(const pmc_maf_t* m, int64_t n, int algo, int fused, pmc_inverse_plan_t* plan) {
    if (!m || !plan || n < 0) return pmc_fail("pmc_maf_inverse_plan: bad argument");
    return pmc_plan_inverse(m, n, algo, fused ? PMC_FUSED_STEP : PMC_FUSED_NO, 1, m->D, plan);
}

// Which sweep PMC_INVERSE_AUTO launches (bench.py names the kernel it times with these; only the subsets depend on the rows)
static int auto_sweep(const pmc_maf_t* m, int64_t n) {
    pmc_inverse_plan_t p;
    return (m && !plan_inverse(m, n, PMC_INVERSE_AUTO, PMC_FUSED_NO, 0, 0, &p)) ? p.sweep : PMC_SWEEP_NONE;
}
extern "C" int pmc_maf_inverse_auto_is_duo(const pmc_maf_t* m, int64_t n) { return auto_sweep(m, n) == PMC_SWEEP_DUO; }
extern "C" int pmc_maf_inverse_auto_is_lane(const pmc_maf_t* m) { return auto_sweep(m, 1) == PMC_SWEEP_LANE; }
extern "C" int pmc_maf_inverse_auto_is_nsf2(const pmc_maf_t* m) { return auto_sweep(m, 1) == PMC_SWEEP_NSF_DUO; }

// ---- which instance of the float32 flow kernels a flow takes (include/pocomc_amd.h: pmc_flow_lds_plan_t)
extern "C" int pmc_maf_lds_plan(const pmc_maf_t* m, pmc_flow_lds_plan_t* plan) {
    if (!m || !plan) return pmc_fail("pmc_maf_lds_plan: bad argument");
    const char* err = nullptr;
    int lean;
    size_t lds = pmc_wg_instance(m, 8, 0, &lean);
    plan->forward_full_bytes = (int32_t)pmc_lds_wg(m, 8, pmc_wg_panel_tiles(m), 0, 0);
    plan->forward_lean = lds ? lean : -1;
    plan->forward_lds_bytes = (int32_t)(lds ? lds : (size_t)plan->forward_full_bytes);
    if (!lds) err = "pmc_maf_forward: flow too wide for 160 KB of LDS";
    lds = pmc_wg_instance(m, 8, 1, &lean);
    plan->dpass_full_bytes = (int32_t)pmc_lds_wg(m, 8, pmc_wg_panel_tiles(m), 1, 0);
    plan->dpass_lean = lds ? lean : -1;
    plan->dpass_lds_bytes = (int32_t)(lds ? lds : (size_t)plan->dpass_full_bytes);
    if (!lds && !err) err = "pmc_maf_forward: flow too wide for 160 KB of LDS";
    size_t full;
    lds = pmc_train_instance(m, &lean, nullptr, &full);
    plan->train_full_bytes = (int32_t)full;
    plan->train_lean = lds ? lean : -1;
    plan->train_lds_bytes = (int32_t)(lds ? lds : full);
    if (!lds && !err) err = "pmc_maf_loss_grad: flow too wide for the 160 KB LDS of one workgroup";
    return err ? pmc_fail(err) : 0;
}
