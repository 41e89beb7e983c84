// Workgroup inverse sweep of the 8-bin spline flows (PMC_INVERSE_TRIANGULAR_WG_NSF -> PMC_SWEEP_WG_NSF; an opt-in, AUTO
// never takes it).  The skeleton, the LDS arrays it works on and the synchronisation contract are in maf_wg_sweep.h: read
// that first.  Here: the kernel, its LDS carve-up and its output stage.  A spline rank has 23 output rows: right-looking
// output accumulators for every rank (the affine kernel's Oacc) would be 161 tiles at D = 102, more than the whole LDS.
// The output stage is therefore LEFT-looking, over the per-rank image parts f3i [rank][half][ktile][lane][4] and b3i
// [rank][32] that the other spline sweeps read:
//
//   H2     [Hp][16]       tiles > J: the skeleton's partial;  tiles <= J: the FINAL h2, written over the slot when the
//                         tile's diagonal phase is over (the partial is dead by then)
//   OP     [NW][16][16]   output partials of the NEXT tile's degree groups, one tile per wavefront (below)
//   PAR [16][32], TAB [16][24]   the rank's 23 parameters and its knot tables (rqs_inverse_coop)
//
//   DIAGONAL phase, after a mini-pass's hidden chain: the rank's two output tiles = its OP tiles, added in slot order,
//       + f3i[g][half][J] h2[J], exchanged through PAR, solved by rqs_inverse_coop: X[g] = x, ladj -= l.  Before the barrier
//       h2[J] goes into H2's slot J.
//   UPDATE phase, after the hidden update: the output partials of tile J + 1's groups, b3i[g] + sum_{K<=J} f3i[g][half][K]
//       H2[K].  A tile has 1-4 groups, so 2-8 (group, half) products of J + 1 fragment products each; they are dealt over
//       the eight wavefronts by (group, half) and, for tiles of one or two groups and products of >= WGN_KSPLIT_MIN K tiles,
//       by four or two K ranges.  Every wavefront writes its own OP tile (the first K range carries the bias); wavefront 0
//       adds the ranges in K order: no atomics, the same bits every call.
//   The partials of tile 0's groups (bias only) are formed before the transform's first barrier.
//
// The contract's "no bound or branch from a value computed from z" holds in the solve too: the spline's bin is picked by
// selects and indexes the row's own PAR / TAB words only (rqs.h).
#include "maf_wg_sweep.h"
#include "rqs.h"

#define WGN_KSPLIT_MIN 16          // K tiles of a (group, half) product from which it is dealt by K range as well: below, the
                                   // product is no longer than the wavefront's hidden update next to it, and unsplit it adds in
                                   // the lone-wave sweep's order (bias, K ascending, diagonal tile) -- flows of one x tile then
                                   // give that sweep's bits (tests/test_gpu_wide_spline_sweep.py)

// acc += sum_{K in [K0, K1)} frag[K] . act[K] in K order on ONE accumulator (mac_range without its second accumulator: the
// order of additions is the lone-wave spline sweep's), the weight fragments of PF K tiles in flight
template <int PF>
__device__ __forceinline__ f32x4 mac_range_seq(f32x4 acc, const float4* __restrict__ frag, const float* act, int K0, int K1, int lane) {
    const int n = K1 - K0;
    if (n <= 0) return acc;
    const float4* f = frag + (size_t)K0 * 64 + lane;
    const float* bp = act + (K0 << 8);
    float4 a[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j) a[j] = f[min(j, n - 1) * 64];
    int k = 0;
    for (; k + PF <= n; k += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const float4 aj = a[j];
            a[j] = f[min(k + j + PF, n - 1) * 64];
            acc = frag_mac(acc, aj, bp + ((k + j) << 8), lane);
        }
    }
#pragma unroll
    for (int j = 0; j < PF - 1; ++j)
        if (k + j < n) acc = frag_mac(acc, a[j], bp + ((k + j) << 8), lane);
    return acc;
}

// The output partial tile of wavefront wv for hidden tile Jn, whose four degree words are dgn: OP[wv] = (first K range:
// b3i[g]) + sum_{K in its range of [0, Kend)} f3i[g][half][K] H2[K].  ng groups -> ns = 4 / 2 / 1 / 1 K ranges per (group,
// half) from WGN_KSPLIT_MIN K tiles on, one below; slot (2 group + half) ns + range.  Returns ns (the same on every wavefront)
template <int NW>
__device__ __forceinline__ int output_partials(const pmc_maf_t& m, const MafView& w, const int (&dgn)[4], int Kend, const float* H2,
                                               float* OP, int wv, int lane) {
    const int q = lane >> 4, p = lane & 15;
    const int D = m.D, nT = m.nT;
    int ng = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = dgn[i];
        if (d < D && (i == 0 || d != dgn[i - 1])) ++ng;
    }
    if (ng == 0) return 1;
    const int ns = Kend < WGN_KSPLIT_MIN ? 1 : ng == 1 ? NW / 2 : ng == 2 ? NW / 4 : NW / 8;
    const int pair = wv / ns, range = wv - pair * ns;
    if (pair >= 2 * ng) return ns;
    int g = 0, seen = 0;                                 // the (pair >> 1)-th group of the tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = dgn[i];
        if (d < D && (i == 0 || d != dgn[i - 1])) {
            if (seen == (pair >> 1)) g = d;
            ++seen;
        }
    }
    const int half = pair & 1;
    const int chunk = (Kend + ns - 1) / ns;
    const int K0 = range * chunk, K1 = min(Kend, K0 + chunk);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (range == 0) acc = bias4(w.b3i, 32 * g + 16 * half + 4 * q);
    acc = mac_range_seq<4>(acc, w.f3i + ((size_t)g * 2 + half) * nT * 64, H2, K0, K1, lane);
    store_rows(OP, wv, q, p, acc);
    return ns;
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void maf_inverse_wg_nsf_sweep_kernel(pmc_maf_t m, const float* __restrict__ in,
                                                                           float* __restrict__ out,
                                                                           float* __restrict__ ladj_out, int64_t n) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane >> 4, p = lane & 15;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    const int D = m.D, Dp = m.Dp, Hp = m.Hp, T = m.T, nT = m.nT, nXT = m.nXT;
    const int nTl = min(m.meta[7], nT);                  // live hidden tiles (the padding tiles trail)
    float* X = smem;
    float* Y = X + Dp * 16;
    float* H1acc = Y + Dp * 16;
    float* H2 = H1acc + Hp * 16;
    float* HT0 = H2 + Hp * 16;
    float* HT1 = HT0 + 256;
    float* HT2 = HT1 + 256;
    float* OP = HT2 + 256;                               // [NW][256]
    float* PAR = OP + NW * 256;                          // [16 rows][32]
    float* TAB = PAR + 16 * 32;                          // [16 rows][24]
    float* RED = TAB + 16 * 24;                          // [NW][16]
    const int* feat_of_rank = m.meta + 8;
    const int* rank_of_feat = m.meta + 8 + T * D;
    const int* quad_meta = m.meta + 8 + 2 * T * D;

    {
        const int* ford = feat_of_rank + (T - 1) * D;
        for (int e = tid; e < Dp * 16; e += 64 * NW) {
            const int r = e >> 4, pp = e & 15;
            float v = 0.0f;
            if (r < D && row0 + pp < n) v = in[(row0 + pp) * D + ford[r]];
            Y[lidx(r, pp)] = v;
            X[lidx(r, pp)] = 0.0f;
        }
    }
    float ladj = 0.0f;                                   // lanes q == 0 of wavefront 0 accumulate their row's log-determinant

    // solve one rank from the accumulators of its two output tiles (wavefront 0; its DS operations execute in order)
#define SOLVE_RANK(G, OA0, OA1)                                                                         \
    {                                                                                                   \
        float* pr_ = PAR + (p << 5) + (q << 2);                                                         \
        *reinterpret_cast<float4*>(pr_) = make_float4(OA0[0], OA0[1], OA0[2], OA0[3]);                  \
        *reinterpret_cast<float4*>(pr_ + 16) = make_float4(OA1[0], OA1[1], OA1[2], OA1[3]);             \
        WAVE_LDS_FENCE();                                                                               \
        float xv_, l_;                                                                                  \
        rqs_inverse_coop(PAR + (p << 5), TAB + p * 24, q, Y[lidx((G), p)], xv_, l_);                    \
        if (q == 0) { X[lidx((G), p)] = xv_; ladj -= l_; }                                              \
        WAVE_LDS_FENCE();                                                                               \
    }

    for (int t = T - 1; t >= 0; --t) {
        const MafView w = maf_view(m, t);
        // the accumulators start from the biases (a thread: one unit, four rows)
        for (int e = tid; e < Hp * 4; e += 64 * NW) {
            const int s = e >> 2, p0 = (e & 3) << 2;
            const float v1 = w.b1[s], v2 = w.b2[s];
#pragma unroll
            for (int j = 0; j < 4; ++j) { H1acc[lidx(s, p0 + j)] = v1; H2[lidx(s, p0 + j)] = v2; }
        }
        int dgn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dgn[i] = __builtin_amdgcn_readfirstlane(quad_meta[i] & 0xffff);
        int ns = output_partials<NW>(m, w, dgn, 0, H2, OP, wv, lane);        // tile 0's groups: bias only
        lds_barrier();
        if (wv == 0) {
            // rank 0 reads nothing: bias only
            const f32x4 o0 = bias4(w.b3i, 4 * q), o1 = bias4(w.b3i, 16 + 4 * q);
            SOLVE_RANK(0, o0, o1)
        }
        // Nothing a tile loads from global memory depends on data: the degree words, wavefront 0's diagonal fragments, layer-0
        // fragments and bias of tile J + 1 are requested while tile J runs, and every wavefront requests the fragments of its
        // hidden update of tile J before the diagonal phase, which it spends waiting at the barrier anyway
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 nfr1 = zero4, nfr2 = zero4, nb0 = zero4, pf0[WGS_PX];
#pragma unroll
        for (int k = 0; k < WGS_PX; ++k) pf0[k] = zero4;
        // per group of the tile: the diagonal fragments of its two output tiles, and the column of W0 of the rank it finds
        float4 fo0[4], fo1[4], col[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { fo0[i] = zero4; fo1[i] = zero4; col[i] = zero4; }
        if (wv == 0) {
            nfr1 = w.f1[lane]; nfr2 = w.f2[lane];
            nb0 = *reinterpret_cast<const float4*>(w.b0 + 4 * q);
#pragma unroll
            for (int k = 0; k < WGS_PX; ++k) pf0[k] = w.f0[(size_t)min(k, nXT - 1) * 64 + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int gi = dgn[i] < D ? dgn[i] : 0;
                fo0[i] = w.f3i[(size_t)gi * 2 * nT * 64 + lane];
                fo1[i] = w.f3i[((size_t)gi * 2 + 1) * nT * 64 + lane];
                col[i] = *reinterpret_cast<const float4*>(w.w0n + (size_t)gi * Hp + 4 * q);
            }
        }
        for (int J = 0; J < nTl; ++J) {
            // the ranks the tile's degree groups produce (D: a padding quad), in slot order
            int dg[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) dg[i] = dgn[i];
            const int Jn = min(J + 1, nT - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) dgn[i] = __builtin_amdgcn_readfirstlane(quad_meta[4 * Jn + i] & 0xffff);

            // ---- the hidden update's fragments: tiles T > J with T mod NW == wv
            const int Tf = J + 1 + ((wv - (J + 1)) & (NW - 1));
            float4 U1[WGS_NU], U2[WGS_NU];
#pragma unroll
            for (int k = 0; k < WGS_NU; ++k) {
                const size_t at = ((size_t)min(Tf + k * NW, nT - 1) * nT + J) * 64 + lane;
                U1[k] = w.f1[at];
                U2[k] = w.f2[at];
            }

            // ---- diagonal phase
            if (wv == 0) {
                const f32x4 p1 = rows_of(H1acc, J, q, p), p2 = rows_of(H2, J, q, p);
                f32x4 a0 = {nb0.x, nb0.y, nb0.z, nb0.w}, a0b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < WGS_PX; ++k) {
                    if (k < nXT) {
                        if (k & 1) a0b = frag_mac(a0b, pf0[k], X + (k << 8), lane);
                        else a0 = frag_mac(a0, pf0[k], X + (k << 8), lane);
                    }
                }
                a0 += a0b;
                a0 = mac_range<4>(a0, w.f0 + (size_t)J * nXT * 64, X, WGS_PX, nXT, lane);
                nb0 = *reinterpret_cast<const float4*>(w.b0 + 16 * Jn + 4 * q);
#pragma unroll
                for (int k = 0; k < WGS_PX; ++k) pf0[k] = w.f0[((size_t)Jn * nXT + min(k, nXT - 1)) * 64 + lane];
                int g_prev = -1, slot = 0;               // slot: the group's first OP tile
                float4 c_prev = zero4;
                f32x4 h2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int g = dg[i];
                    const bool group = g < D && (i == 0 || g != dg[i - 1]);
                    if (!group && !(i == 3 && g_prev < 0)) continue;        // (a tile without a group: its units once)
                    if (g_prev >= 0) {
                        // the rank the last mini-pass found enters layer 0: one column of W0
                        const float xv = X[lidx(g_prev, p)];
                        a0[0] += c_prev.x * xv; a0[1] += c_prev.y * xv; a0[2] += c_prev.z * xv; a0[3] += c_prev.w * xv;
                    }
                    f32x4 h0, a1;
#pragma unroll
                    for (int r = 0; r < 4; ++r) h0[r] = fmaxf(a0[r], 0.0f);
                    store_rows(HT0, 0, q, p, h0);
                    WAVE_LDS_FENCE();
                    a1 = frag_mac(p1, nfr1, HT0, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) a1[r] = fmaxf(a1[r] + h0[r], 0.0f);
                    store_rows(HT1, 0, q, p, a1);
                    WAVE_LDS_FENCE();
                    h2 = frag_mac(p2, nfr2, HT1, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) h2[r] = fmaxf(h2[r] + a1[r], 0.0f);
                    store_rows(HT2, 0, q, p, h2);
                    WAVE_LDS_FENCE();
                    if (group) {
                        // the K ranges of the two output tiles in K order, then the diagonal tile
                        f32x4 o0 = rows_of(OP, slot, q, p), o1 = rows_of(OP, slot + ns, q, p);
                        for (int s = 1; s < ns; ++s) {
                            o0 += rows_of(OP, slot + s, q, p);
                            o1 += rows_of(OP, slot + ns + s, q, p);
                        }
                        o0 = frag_mac(o0, fo0[i], HT2, lane);
                        o1 = frag_mac(o1, fo1[i], HT2, lane);
                        SOLVE_RANK(g, o0, o1)
                        slot += 2 * ns;
                        g_prev = g;
                        c_prev = col[i];
                    }
                }
                store_rows(H2, J, q, p, h2);             // final: what the output partials of every later tile read
                nfr1 = w.f1[((size_t)Jn * nT + Jn) * 64 + lane];
                nfr2 = w.f2[((size_t)Jn * nT + Jn) * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int gi = dgn[i] < D ? dgn[i] : 0;
                    fo0[i] = w.f3i[(((size_t)gi * 2) * nT + Jn) * 64 + lane];
                    fo1[i] = w.f3i[(((size_t)gi * 2 + 1) * nT + Jn) * 64 + lane];
                    col[i] = *reinterpret_cast<const float4*>(w.w0n + (size_t)gi * Hp + 16 * Jn + 4 * q);
                }
            }
            lds_barrier();

            // ---- update phase: tile J is final
#pragma unroll
            for (int k = 0; k < WGS_NU; ++k) {
                const int Tt = Tf + k * NW;
                if (Tt < nTl) {
                    f32x4 a1 = rows_of(H1acc, Tt, q, p), a2 = rows_of(H2, Tt, q, p);
                    a1 = frag_mac(a1, U1[k], HT0, lane);
                    a2 = frag_mac(a2, U2[k], HT1, lane);
                    store_rows(H1acc, Tt, q, p, a1);
                    store_rows(H2, Tt, q, p, a2);
                }
            }
            for (int Tt = Tf + WGS_NU * NW; Tt < nTl; Tt += NW) {            // (flows of more than 8 WGS_NU + 1 hidden tiles)
                const size_t at = ((size_t)Tt * nT + J) * 64 + lane;
                f32x4 a1 = rows_of(H1acc, Tt, q, p), a2 = rows_of(H2, Tt, q, p);
                a1 = frag_mac(a1, w.f1[at], HT0, lane);
                a2 = frag_mac(a2, w.f2[at], HT1, lane);
                store_rows(H1acc, Tt, q, p, a1);
                store_rows(H2, Tt, q, p, a2);
            }
            if (J + 1 < nTl) ns = output_partials<NW>(m, w, dgn, J + 1, H2, OP, wv, lane);
            lds_barrier();
        }
        // x of this transform is the next one's input (by that transform's ranks), or the result; X starts from zero again
        {
            const int* ford = feat_of_rank + t * D;
            const int* rnext = t > 0 ? rank_of_feat + (t - 1) * D : nullptr;
            for (int e = tid; e < Dp * 16; e += 64 * NW) {
                const int r = e >> 4, pp = e & 15;
                if (r < D) {
                    const float v = X[lidx(r, pp)];
                    const int feat = ford[r];
                    if (rnext) Y[lidx(rnext[feat], pp)] = v;
                    else if (row0 + pp < n) out[(row0 + pp) * D + feat] = v;
                }
                X[lidx(r, pp)] = 0.0f;
            }
        }
    }
#undef SOLVE_RANK
    const float l = quad_sum(ladj);
    if (lane < 16) RED[wv * 16 + lane] = l;
    lds_barrier();
    if (wv == 0) {
        float lt = 0.0f;
#pragma unroll
        for (int k = 0; k < NW; ++k) lt += RED[16 * k + p];
        if (ladj_out && lane < 16 && row0 + p < n) ladj_out[row0 + p] = lt;
    }
}

// The instance the plan names (inverse_plan.hip: PMC_SWEEP_WG_NSF): the plain inverse of z only
int pmc_launch_inverse_wg_nsf_sweep(const pmc_inverse_plan_t* plan, const ProposeArgs* pa, const pmc_maf_t* m, const float* z,
                                    float* x, float* ladj, int64_t n, hipStream_t stream) {
    const size_t lds = pmc_lds_wg_nsf_sweep(m);
    if (plan->sweep != PMC_SWEEP_WG_NSF || pa || m->n_out != 23 || !m->tri_ok || lds > PMC_LDS_CAP || (size_t)plan->lds_bytes != lds)
        return pmc_fail("pmc_launch_inverse_wg_nsf_sweep: not this sweep's plan");
    if (int e = pmc_launch_lds(maf_inverse_wg_nsf_sweep_kernel<WGS_NW>, "hipFuncSetAttribute(maf_inverse_wg_nsf_sweep_kernel)",
                               dim3((unsigned)((n + 15) / 16)), dim3(64 * WGS_NW), lds, stream, *m, z, x, ladj, n)) return e;
    return pmc_check_launch("maf_inverse_wg_nsf_sweep_kernel");
}
