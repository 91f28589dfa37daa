/* sph.hip — SPH density (with the smoothing-length iteration) and hydro force for gfx950.
 *
 * Replaces treewalk_primary_kernel<DensityTreeWalk*> / <HydroTreeWalk*> (treewalk2.cuh:104-134,
 * densitycuda.cu, hydracuda.cu) AND the host-side Hsml loop the reference keeps on the CPU
 * (TreeWalk::do_hsml_loop, treewalk2.h:480-557; DensityOutput::postprocess +
 * density_check_neighbours, densitytree2.hpp:117-257; queue compaction).
 *
 * Structure (same wavefront-collective walk as grav_walk.hip):
 *   - a wavefront owns 64 consecutive targets of the work queue; the union of the lanes'
 *     neighbour walks is traversed with a wave-uniform `cur` and per-lane `mynext`; the cull
 *     test (cull_node, localtreewalk2.h:154-182) is evaluated per lane, so every target sees
 *     exactly the candidate set the reference's walk gives it, in the same order;
 *   - per-neighbour quantities that the reference recomputes for every pair (SPH_VelPred,
 *     SPH_EntVarPred, density/pressure prediction, sound speed, the Balsara factor f2 of j) are
 *     pure functions of particle j, so a prepass evaluates them once per particle and stores them
 *     in leaf order;
 *   - node records and candidate particles are staged through LDS (64-node window of the pre-order
 *     pool, 64-candidate tile) and accepted neighbours go to per-lane lists that are evaluated lane
 *     by lane (see ngb_walk below);
 *   - the Hsml iteration runs on the device: walk -> postprocess (bisection / Newton step,
 *     Left/Right brackets) -> order-preserving compaction of the redo queue; the host only reads
 *     back the queue length once per iteration.
 * All arithmetic is f64.
 * The walk itself (ngb_walk and its one-wave / one-workgroup variants) is in sph_walk.hpp, shared with the other neighbour
 * operators (sph_ngbsums.hip, sph_bh.hip, sph_winds.hip); the small kernels and host helpers they share are defined here.
 */
#include "sph_walk.hpp"
#include <string.h>

namespace {

/* KickFactorData::SPH_EntVarPred, density2.h:115-128 */
__device__ __forceinline__ double entvar_pred(double Entropy, double DtEntropy, double dloga)
{
    double e = Entropy + DtEntropy * dloga;
    if(e < 0.05 * Entropy)
        e = 0.05 * Entropy;
    if(e <= 0)
        return 0;
    return exp(1. / SPH_GAMMA * log(e));
}
/* SPH_DensityPred, hydratree2.hpp:21-34 */
__device__ __forceinline__ double density_pred(double Density, double DivVel, double dtdrift)
{
    const double d = Density - DivVel * Density * dtdrift;
    return (d >= 1e-6 * Density) ? d : 1e-6 * Density;
}
/* PressurePredict, hydratree2.hpp:47-58 */
__device__ __forceinline__ double pressure_predict(double eom, double evp)
{
    if(evp * eom <= 0)
        return 0;
    return exp(SPH_GAMMA * log(evp * eom));
}

/* ---- prepass: per-particle predicted quantities -------------------------------------------- */
struct PredArgs {
    long long n;
    const uint8_t *pflags;
    const double *vel, *treeacc, *gravpm, *hydroaccel; /* [N][3] by particle index */
    const uint8_t *bin_grav, *bin_hydro;
    const double *entropy, *dtentropy;
    const double *hsml;
    const double *density, *egywt, *dhsmlegy, *divvel, *curlvel;
    double4 *velp, *hydC, *hydD;
    const double *evp_in; /* caller-provided EntVarPred by particle index, or null */
    shq_kick_factors kf;
    double drifts[SHQ_TIMEBINS + 1];
    int hydro;          /* also fill hydC/hydD */
    int DISPH;
    double fac_mu, contrast;
};

__global__ void sph_predict_kernel(const PredArgs a)
{
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= a.n)
        return;
    const int type = a.pflags[i] >> 4;
    if(type != 0) {
        /* non-gas (BH targets use their own velocity: DensityQuery ctor, densitytree2.hpp:270-277) */
        a.velp[i] = make_double4(a.vel[3 * i], a.vel[3 * i + 1], a.vel[3 * i + 2], 0.0);
        return;
    }
    const int bg = a.bin_grav[i], bh = a.bin_hydro[i];
    /* SPH_VelPred, density2.h:89-98 */
    double v[3];
    for(int j = 0; j < 3; j++)
        v[j] = a.vel[3 * i + j] + a.kf.gravkicks[bg] * a.treeacc[3 * i + j] + a.gravpm[3 * i + j] * a.kf.FgravkickB +
               a.kf.hydrokicks[bh] * a.hydroaccel[3 * i + j];
    const double evp = a.evp_in ? a.evp_in[i] : entvar_pred(a.entropy[i], a.dtentropy[i], a.kf.dloga_kick[bh]);
    a.velp[i] = make_double4(v[0], v[1], v[2], evp);
    if(a.hydro) {
        /* ngbiter's j-side quantities, hydratree2.hpp:283-300,325-326,357-364 */
        const double density_j = density_pred(a.density[i], a.divvel[i], a.drifts[bh]);
        const double eom_j = density_pred(a.DISPH ? a.egywt[i] : a.density[i], a.divvel[i], a.drifts[bh]);
        const double P = pressure_predict(eom_j, evp);
        const double cs = sqrt(SPH_GAMMA * P / eom_j);
        a.hydC[i] = make_double4(evp, density_j, cs, P / (eom_j * eom_j));
        const double f2 = fabs(a.divvel[i]) / (fabs(a.divvel[i]) + a.curlvel[i] + 0.0001 * cs / a.fac_mu / a.hsml[i]);
        double rr2 = 1;
        if(a.DISPH) {
            rr2 = 0;
            if(a.contrast >= 0) {
                rr2 = eom_j / density_j;
                if(a.contrast > 0)
                    rr2 = fmin(rr2, a.contrast);
            }
        }
        a.hydD[i] = make_double4(a.dhsmlegy[i], rr2, f2, a.kf.dloga_for_bin[bh]);
    }
}

__global__ void sph_gather_leaf_kernel(long long nleaf, const int32_t *pidx, const double4 *velp, const double4 *hydC,
                                       const double4 *hydD, const double *hsml, const uint8_t *pflags, const double *delay,
                                       double4 *velp_leaf, HydRec *hydrec_leaf, double *hsml_leaf,
                                       int32_t *flag_leaf, const double4 *posm_leaf = nullptr, float4 *posf_leaf = nullptr, double pre_eps = 0)
{
    const long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(s >= nleaf)
        return;
    const int p = pidx[s];
    velp_leaf[s] = velp[p];
    if(hydrec_leaf) {
        HydRec r;
        const double4 v = velp[p];
        r.posm = posm_leaf[s];
        r.velh = make_double4(v.x, v.y, v.z, hsml[p]);
        r.C = hydC[p];
        r.D = hydD[p];
        hydrec_leaf[s] = r;
    }
    hsml_leaf[s] = hsml[p];
    const uint8_t f = pflags[p];
    uint8_t o = 0;
    if((f & 1) || (f >> 4) != 0) /* IsGarbage, or type changed since the tree was built (GASMASK) */
        o |= 1;
    if(delay && delay[p] > 0)
        o |= 2;
    flag_leaf[s] = o;
    if(posf_leaf) {
        const double4 q = posm_leaf[s];
        float4 f = make_float4((float) q.x, (float) q.y, (float) q.z, pre32_bound(hsml[p], pre_eps));
        if(o & 1)
            f.x = __builtin_nanf("");             /* not a candidate at all */
        else if(hydrec_leaf && (o & 2))
            f.x = __builtin_inff();               /* hydro never accepts a wind-decoupled particle (it still counts as a candidate) */
        posf_leaf[s] = f;
    }
}

/* per leaf node: how many of its particles the scans pass over (flag bit 0), kept at the leaf's first slot: the f32 scan takes a
 * leaf's candidate count from its node and subtracts this */
__global__ void sph_leaf_ngarb_kernel(int npool, const NodeC *__restrict__ nodeC, const int32_t *__restrict__ flag_leaf, int32_t *ngarb_leaf)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= npool)
        return;
    const NodeC nc = nodeC[i];
    if(nc.type != SHQ_PARTICLE_NODE_TYPE || nc.count <= 0)
        return;
    int ng = 0;
    for(int j = 0; j < nc.count; j++)
        ng += flag_leaf[nc.child + j] & 1;
    ngarb_leaf[nc.child] = ng;
}

/* MODE 0: fused walk + evaluation (persistent grid, one list region per resident wave; also the redo path:
 * d_nq != NULL takes the queue length from the device).  MODE 1: walk only, lists and their lengths go to
 * global memory (one region per wave of the launch).  MODE 2: evaluation only, from those lists.  MODE 3: one target
 * per wave (heavy_walk) for the targets whose list did not fit; launched with 64 threads per block.  The
 * two-kernel path lets the walk run at twice the occupancy the register-heavy evaluation allows. */
template <int KT, int MODE, bool GHOSTS>
__device__ __forceinline__ void sph_density_body(const SphDev &a, const int32_t *queue, long long nq, int WindsDecouple,
                                                 unsigned long long *nint_total, int32_t *__restrict__ nlist, long long ntasks,
                                                 int32_t *__restrict__ counts, const long long *d_nq, const int4 *qseg)
{
    __shared__ __attribute__((aligned(32))) char lds[MODE == 4 ? sizeof(HbShared) : (MODE == 3 ? HW_LDS : (MODE == 2 ? 1 : (MODE == 1 ? SPH_WALK_WPB : 4) * NW_LDS_PER_WAVE(false)))];
    const int lane = threadIdx.x & 63;
    if((MODE == 0 || MODE >= 3) && d_nq) {
        nq = *d_nq;
        ntasks = MODE >= 3 ? nq : (nq + 255) / 256;
    }
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = MODE == 4 ? task : task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + (MODE == 0 ? ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) : (size_t) wave) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = MODE >= 3 ? wave : wave * 64 + lane; /* MODE 3 / 4: every lane of the wave / workgroup works for the same target */
    bool valid = t < nq;
    long long pi = 0;
    double px = 0, py = 0, pz = 0, h = 0, vx = 0, vy = 0, vz = 0;
    int type = 0;
    if(valid) {
        pi = queue ? (long long) queue[t] : t;
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z;
        h = a.hsml[pi];
        const double4 v = a.velp[pi];
        vx = v.x; vy = v.y; vz = v.z;
        type = a.pflags[pi] >> 4;
    }
    const Kern<KT> kernel(valid ? h : 1.0);
    const double h2 = h * h, Hinv = 1.0 / kernel.H, vol = kernel.volume();
    const bool nowind = WindsDecouple && type == 5; /* wind-decoupled neighbours are invisible to black holes */
    double Ngb = 0, Rho = 0, DhsmlDensity = 0, EgyRho = 0, DhsmlEgy = 0, Div = 0;
    double R0 = 0, R1 = 0, R2 = 0, G0 = 0, G1 = 0, G2 = 0;

    /* ngbiter, densitytree2.hpp:362-423; dist points from the neighbour to the target */
    auto pair = [&](const int s) {
        const double4 q = a.posm_leaf[s];
        const double4 w = a.velp_leaf[s];
        const double d0 = wrapd(px - q.x, a.Box, a.invBox);
        const double d1 = wrapd(py - q.y, a.Box, a.invBox);
        const double d2 = wrapd(pz - q.z, a.Box, a.invBox);
        const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
        /* the lists of the f32 pre-test hold a superset: the reference's test (densitytree2.hpp:362-375) decides here */
        if(!(r2 < h2) || (nowind && (a.flag_leaf[s] & 2)))
            return;
        const double r = sqrt(r2);
        const double u = r * Hinv;
        const double wk = kernel.wk(u);
        const double dwk = kernel.dwk(u);
        Ngb += wk * vol;
        const double mj = q.w;
        Rho += mj * wk;
        const double dW = -(3 * wk * Hinv + u * dwk); /* DensityKrnl::dW, densitykernel.hpp:58-61 */
        DhsmlDensity += mj * dW;
        EgyRho += mj * w.w * wk;
        DhsmlEgy += mj * w.w * dW;
        if(r > 0) {
            const double fac = mj * dwk / r;
            const double e0 = vx - w.x, e1 = vy - w.y, e2 = vz - w.z;
            Div += -fac * (d0 * e0 + d1 * e1 + d2 * e2);
            R0 += fac * (e1 * d2 - e2 * d1);
            R1 += fac * (e2 * d0 - e0 * d2);
            R2 += fac * (e0 * d1 - e1 * d0);
            G0 += fac * d0;
            G1 += fac * d1;
            G2 += fac * d2;
        }
    };

    auto accept = [&](const double r2, const double, const int fl) { return r2 < h2 && !(nowind && (fl & 2)); };
    unsigned int nint = 0;
    int fill = 0;
    bool ovf = false;
    if(MODE == 4) {
        HbShared &sh = *reinterpret_cast<HbShared *>(lds);
        nint = heavy_block<false>(a, sh, px, py, pz, h, accept, pair);
        Ngb = hb_sum(Ngb, sh.red); Rho = hb_sum(Rho, sh.red); DhsmlDensity = hb_sum(DhsmlDensity, sh.red); EgyRho = hb_sum(EgyRho, sh.red);
        DhsmlEgy = hb_sum(DhsmlEgy, sh.red); Div = hb_sum(Div, sh.red); R0 = hb_sum(R0, sh.red); R1 = hb_sum(R1, sh.red); R2 = hb_sum(R2, sh.red);
        G0 = hb_sum(G0, sh.red); G1 = hb_sum(G1, sh.red); G2 = hb_sum(G2, sh.red);
        valid = threadIdx.x == 0;
    } else if(MODE == 3) {
        bool aborted = false;
        nint = heavy_walk<false>(a, lds, px, py, pz, h, accept, pair, aborted);
        if(aborted) { /* too much for one wave: a whole workgroup takes it */
            if(lane == 0)
                a.heavy2[atomicAdd((unsigned long long *) a.nheavy2, 1ull)] = (int32_t) pi;
            continue;
        }
        Ngb = wave_sum(Ngb); Rho = wave_sum(Rho); DhsmlDensity = wave_sum(DhsmlDensity); EgyRho = wave_sum(EgyRho); DhsmlEgy = wave_sum(DhsmlEgy);
        Div = wave_sum(Div); R0 = wave_sum(R0); R1 = wave_sum(R1); R2 = wave_sum(R2); G0 = wave_sum(G0); G1 = wave_sum(G1); G2 = wave_sum(G2);
        valid = lane == 0;
    } else if(MODE != 2)
        nint = ngb_walk<false, MODE == 1, GHOSTS, true>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(false), myl, valid, px, py, pz, h, accept, pair,
                                                        (unsigned int *) nullptr, fill, ovf,
                                                        (GHOSTS && valid) ? qseg[t] : make_int4(-1, -1, -1, -1),
                                                        valid ? pre32_bound(h, a.Box * 0x1p-20) : 0.f);
    if(MODE == 1) {
        counts[wave * 64 + lane] = ovf ? -1 : fill; /* -1: this target goes to the one-target-per-wave kernel */
        if(ovf)
            nint = 0; /* counted there */
    }
    if(MODE == 2) {
        fill = counts[wave * 64 + lane];
        if(fill < 0) { /* walked on its own (MODE 3) */
            fill = 0;
            valid = false;
        }
        nl_flush(myl, fill, pair);
    }
    if(MODE != 1 && valid) {
        /* DensityResult::reduce<PRIMARY>, densitytree2.hpp:308-343 */
        a.numngb[pi] = Ngb;
        a.dhsmldens[pi] = DhsmlDensity;
        a.rho[pi] = Rho;
        a.div[pi] = Div;
        if(type == 0 || GHOSTS) { /* an imported query returns every sum; its owner's reduce picks by type */
            a.rot[3 * pi] = R0;
            a.rot[3 * pi + 1] = R1;
            a.rot[3 * pi + 2] = R2;
            if(a.gradrho) {
                a.gradrho[3 * pi] = G0;
                a.gradrho[3 * pi + 1] = G1;
                a.gradrho[3 * pi + 2] = G2;
            }
            a.egyrho[pi] = EgyRho;
            a.dhsmlegy[pi] = DhsmlEgy;
        }
    }
    unsigned int sn = nint;
    for(int off = 32; off > 0; off >>= 1)
        sn += __shfl_xor(sn, off);
    if(lane == 0 && nint_total)
        atomicAdd(nint_total, (unsigned long long) sn);
    } /* task loop */
}

template <int KT, int MODE, bool GHOSTS = false>
__global__ __launch_bounds__(256) void sph_density_kernel(const SphDev a, const int32_t *queue, long long nq, int WindsDecouple,
                                                          unsigned long long *nint_total, int32_t *__restrict__ nlist, long long ntasks,
                                                          int32_t *__restrict__ counts, const long long *d_nq, const int4 *qseg = nullptr)
{
    sph_density_body<KT, MODE, GHOSTS>(a, queue, nq, WindsDecouple, nint_total, nlist, ntasks, counts, d_nq, qseg);
}

/* MODE 4: one target per workgroup of 512 threads */
template <int KT>
__global__ __launch_bounds__(HB_THREADS) void sph_density_block_kernel(const SphDev a, const int32_t *queue, int WindsDecouple,
                                                                       unsigned long long *nint_total, const long long *d_nq)
{
    sph_density_body<KT, 4, false>(a, queue, 0, WindsDecouple, nint_total, nullptr, 0, nullptr, d_nq, nullptr);
}

/* ---- density postprocess + Hsml update (DensityOutput::postprocess, density_check_neighbours) -- */
struct PostArgs {
    double Box, DesNumNgb, DesNumNgbBH, MinGasHsml, MaxDev;
    int update_hsml, BlackHoleOn, DoEgyDensity;
    unsigned long long *hmax_tried; /* the largest Hsml any walk of this loop has run with or any target ends with, as the bits of a non-negative double */
};

__global__ void sph_density_post_kernel(const SphDev a, const int32_t *queue, long long nq, const PostArgs p, int32_t *todo)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nq)
        return;
    const long long i = queue ? (long long) queue[t] : t;
    const int type = a.pflags[i] >> 4;
    int done = 0;
    const double density = a.rho[i];
    double hs = a.hsml[i];
    /* the radius the walk behind this call searched: a sharded caller's halo must cover the largest one TRIED, not just the one the
     * loop ends with (an intermediate guess that reaches past the imported ghosts undercounts NumNgb and steers the next guess) */
    if(p.hmax_tried && (unsigned long long) __double_as_longlong(hs) > *(volatile unsigned long long *) p.hmax_tried)
        atomicMax(p.hmax_tried, (unsigned long long) __double_as_longlong(hs));
    double DhsmlDens = a.dhsmldens[i];
    DhsmlDens *= hs / (3 * density);
    DhsmlDens = 1 / (1 + DhsmlDens);
    a.dhsmldens[i] = DhsmlDens;
    if(p.update_hsml) {
        double desnumngb = p.DesNumNgb;
        if(p.BlackHoleOn && type == 5)
            desnumngb = p.DesNumNgbBH;
        const double NumNgb = a.numngb[i];
        double L = a.left[i], R = a.right[i];
        if(NumNgb < (desnumngb - p.MaxDev) || (NumNgb > (desnumngb + p.MaxDev))) {
            if((R - L) < 1.0e-5 * R) {
                hs = R;
                done = 1;
            } else {
                if(NumNgb < desnumngb)
                    L = hs;
                else
                    R = hs;
                if((R < p.Box && L > 0) || (hs * 1.26 > 0.99 * p.Box))
                    hs = cbrt(0.5 * (L * L * L + R * R * R));
                else {
                    const double DensFac = DhsmlDens;
                    double fac = 1.26;
                    if(NumNgb > 0)
                        fac = 1 - (NumNgb - desnumngb) / (3 * NumNgb) * DensFac;
                    if(R > 0.99 * p.Box && L > 0)
                        if(DensFac <= 0 || fabs(NumNgb - desnumngb) >= 0.5 * desnumngb || fac > 1.26)
                            fac = 1.26;
                    if(R < 0.99 * p.Box && L == 0)
                        if(DensFac <= 0 || fac < 1. / 3)
                            fac = 1. / 3;
                    hs *= fac;
                }
                if(R < p.MinGasHsml) {
                    hs = p.MinGasHsml;
                    done = 1;
                } else
                    done = 0;
            }
            a.left[i] = L;
            a.right[i] = R;
        } else {
            if(hs < p.MinGasHsml)
                hs = p.MinGasHsml;
            done = 1;
        }
        a.hsml[i] = hs;
        /* a target can end on a radius no walk ran with: the collapsed bracket leaves Right (Box itself for a target alone in the box),
         * the floors leave MinGasHsml.  The next operator searches with it, so the report covers it too */
        if(done && p.hmax_tried && (unsigned long long) __double_as_longlong(hs) > *(volatile unsigned long long *) p.hmax_tried)
            atomicMax(p.hmax_tried, (unsigned long long) __double_as_longlong(hs));
    }
    if(type == 0) {
        if(p.DoEgyDensity) {
            const double EntPred = a.velp[i].w;
            double d = a.dhsmlegy[i];
            d *= hs / (3 * a.egyrho[i]);
            d *= -DhsmlDens;
            a.dhsmlegy[i] = d;
            a.egyrho[i] = a.egyrho[i] / EntPred;
        } else
            a.dhsmlegy[i] = DhsmlDens;
        const double r0 = a.rot[3 * i], r1 = a.rot[3 * i + 1], r2 = a.rot[3 * i + 2];
        a.curl[i] = sqrt(r0 * r0 + r1 * r1 + r2 * r2) / density;
        const double dv = a.div[i] / density;
        a.div[i] = dv;
        a.dthsml[i] = (1.0 / 3) * dv * hs;
    } else if(type == 5) {
        const double dv = a.div[i] / density;
        a.div[i] = dv;
        a.dthsml[i] = (1.0 / 3) * dv * hs;
    }
    if(todo)
        todo[t] = done ? -1 : (int32_t) i;
    if(done && p.update_hsml && type == 0 && a.pfather) {
        /* update_tree_hmax_father, forcetree.cpp:1285-1313; non-negative doubles order like their bits */
        const int no = a.pfather[i];
        if(no >= 0) {
            const NodeB B = a.nodeB[no];
            const double4 P = a.posm[i];
            double nh = 0;
            nh = fmax(nh, fabs(P.x - B.center[0]) + hs - B.len / 2.);
            nh = fmax(nh, fabs(P.y - B.center[1]) + hs - B.len / 2.);
            nh = fmax(nh, fabs(P.z - B.center[2]) + hs - B.len / 2.);
            atomicMax(reinterpret_cast<unsigned long long *>(&a.hmax[no]), (unsigned long long) __double_as_longlong(nh));
        }
    }
}

/* ---- order-preserving compaction of the redo queue (three small kernels) --------------------------- */
__global__ void compact_count_kernel(const int32_t *todo, long long n, int32_t *blockcount)
{
    __shared__ int s;
    if(threadIdx.x == 0)
        s = 0;
    __syncthreads();
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    const bool f = (t < n) && (todo[t] >= 0);
    const unsigned long long m = shq_ballot(f);
    if((threadIdx.x & 63) == 0)
        atomicAdd(&s, __popcll(m));
    __syncthreads();
    if(threadIdx.x == 0)
        blockcount[blockIdx.x] = s;
}
__global__ void compact_scan_kernel(int32_t *blockcount, int nblocks, long long *total)
{
    /* single workgroup exclusive scan */
    __shared__ long long carry;
    __shared__ int buf[1024];
    if(threadIdx.x == 0)
        carry = 0;
    __syncthreads();
    for(int base = 0; base < nblocks; base += 1024) {
        const int i = base + threadIdx.x;
        const int v = (i < nblocks) ? blockcount[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for(int off = 1; off < 1024; off <<= 1) {
            int add = (threadIdx.x >= off) ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        const int incl = buf[threadIdx.x];
        if(i < nblocks)
            blockcount[i] = (int32_t) (carry + incl - v);
        __syncthreads();
        if(threadIdx.x == 1023)
            carry += incl;
        __syncthreads();
    }
    if(threadIdx.x == 0)
        *total = carry;
}
__global__ void compact_write_kernel(const int32_t *todo, long long n, const int32_t *blockoff, int32_t *out)
{
    __shared__ int wavebase[4];
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    const bool f = (t < n) && (todo[t] >= 0);
    const unsigned long long m = shq_ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if(lane == 0)
        wavebase[w] = __popcll(m);
    __syncthreads();
    int base = blockoff[blockIdx.x];
    for(int k = 0; k < w; k++)
        base += wavebase[k];
    if(f) {
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        out[base + rank] = todo[t];
    }
}

/* ---- hydro walk (HydroLocalTreeWalk::ngbiter, hydratree2.hpp:253-378) ----------------------------- */
struct HydroConst {
    double hubble_a2, fac_mu, fac_vsic_fix, ArtBulkViscConst, contrast;
    int DISPH;
};

/* MODE as for sph_density_kernel */
template <int KT, int MODE, bool GHOSTS>
__device__ __forceinline__ void sph_hydro_body(const SphDev &a, const int32_t *queue, long long nq, const HydroConst &hc,
                                               unsigned long long *nint_total, int32_t *__restrict__ nlist, long long ntasks,
                                               int32_t *__restrict__ counts, const long long *d_nq, const int4 *qseg)
{
    __shared__ __attribute__((aligned(32))) char lds[MODE == 4 ? sizeof(HbShared) : (MODE == 3 ? HW_LDS : (MODE == 2 ? 1 : (MODE == 1 ? SPH_WALK_WPB : 4) * NW_LDS_PER_WAVE(true)))];
    const int lane = threadIdx.x & 63;
    if((MODE == 0 || MODE >= 3) && d_nq) {
        nq = *d_nq;
        ntasks = MODE >= 3 ? nq : (nq + 255) / 256;
    }
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = MODE == 4 ? task : task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + (MODE == 0 ? ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) : (size_t) wave) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = MODE >= 3 ? wave : wave * 64 + lane; /* MODE 3 / 4: every lane of the wave / workgroup works for the same target */
    bool valid = t < nq;
    long long pi = 0;
    double px = 0, py = 0, pz = 0, mi = 0, hi = 1, vx = 0, vy = 0, vz = 0;
    double4 Ci = make_double4(1, 1, 1, 1), Di = make_double4(0, 0, 0, 0);
    if(valid) {
        pi = queue ? (long long) queue[t] : t;
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z; mi = p.w;
        hi = a.hsml[pi];
        const double4 v = a.velp[pi];
        vx = v.x; vy = v.y; vz = v.z;
        Ci = a.hydC[pi];
        Di = a.hydD[pi];
    }
    /* HydroQuery ctor, hydratree2.hpp:165-191: for the target itself the un-drifted values apply, but a
     * target is active, so its drift factor is zero and the predicted values coincide. */
    const double iEntVarPred = Ci.x, iDensity = Ci.y, soundspeed_i = Ci.z, p_over_rho2_i = Ci.w;
    const double iDhsml = Di.x, iF1 = Di.z, idloga = Di.w;
    /* rr1 = EgyRho / Density with the contrast limit; Di.y holds exactly that for the target */
    const double rr1 = Di.y;
    const Kern<KT> kernel_i(hi);
    const double hi2 = hi * hi;
    const double si = (Kern<KT>::support / 2.) / hi, dnorm_i = kernel_i.dnorm, inv_iEVP = 1.0 / iEntVarPred;
    double A0 = 0, A1 = 0, A2 = 0, DtE = 0;
    double MaxSig = soundspeed_i; /* HydroResult ctor: sqrt(GAMMA P / EgyRho) */

    /* HydroLocalTreeWalk::ngbiter, hydratree2.hpp:253-378, for one accepted neighbour (leaf slot s) */
    auto pair = [&](const int s) {
        const HydRec *rec = a.hydrec_leaf + s;
        const double4 q = rec->posm;
        const double4 w = rec->velh;
        const double4 Cj = rec->C;
        const double4 Dj = rec->D;
        const double hj = w.w;
        const double d0 = wrapd(px - q.x, a.Box, a.invBox);
        const double d1 = wrapd(py - q.y, a.Box, a.invBox);
        const double d2 = wrapd(pz - q.z, a.Box, a.invBox);
        const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
        /* the lists of the f32 pre-test hold a superset: the reference's test (hydratree2.hpp:253-262) decides here (a wind-decoupled
         * particle never reaches a list: its f32 record is at infinity, and the f64 scan's accept() knows its flag) */
        if(!(r2 > 0 && (r2 < hi2 || r2 < hj * hj)))
            return;
        /* The reference divides by r, H and the entropy variables at every use; with ~10 f64 divisions
         * (a dozen instructions each) they were half of this function.  Here 1/r comes from v_rsq_f64 + a
         * Newton step and the kernel of j from one reciprocal of h_j: same formulas, results differ from
         * the oracle's at the 1e-16 level. */
        const double EVP = Cj.x, density_j = Cj.y, soundspeed_j = Cj.z, p_over_rho2_j = Cj.w;
        double vsig = soundspeed_i + soundspeed_j;
        if(vsig > MaxSig)
            MaxSig = vsig;
        const double e0 = vx - w.x, e1 = vy - w.y, e2 = vz - w.z;
        const double vdotr = d0 * e0 + d1 * e1 + d2 * e2;
        const double vdotr2 = vdotr + hc.hubble_a2 * r2;
        const double y0 = __builtin_amdgcn_rsq(r2);
        const double ye = fma(-r2 * y0, y0, 1.0);
        const double rinv = fma(y0 * ye, fma(ye, 0.375, 0.5), y0);
        const double r = r2 * rinv;
        const double sj = (Kern<KT>::support / 2.) / hj; /* q = r * support / (2 H) */
        const double sigma = (KT == 1) ? (1 / M_PI) : ((KT == 2) ? (1 / (120 * M_PI)) : (1 / (20 * M_PI)));
        const double dnorm_j = sigma * (sj * sj) * (sj * sj);
        const double dwk_i = dnorm_i * kernel_i.dwk_int(r * si);
        const double dwk_j = dnorm_j * kernel_i.dwk_int(r * sj);
        double visc = 0;
        if(vdotr2 < 0) {
            const double mu_ij = hc.fac_mu * vdotr2 * rinv;
            const double rho_ij = 0.5 * (iDensity + density_j);
            vsig = soundspeed_i + soundspeed_j - 3 * mu_ij;
            if(vsig > MaxSig)
                MaxSig = vsig;
            visc = 0.25 * hc.ArtBulkViscConst * vsig * (-mu_ij) / rho_ij * (iF1 + Dj.z);
            const double dloga = 2 * fmax(idloga, Dj.w);
            if(dloga > 0 && (dwk_i + dwk_j) < 0) {
                if((mi + q.w) > 0)
                    visc = fmin(visc, 0.5 * hc.fac_vsic_fix * vdotr2 / (0.5 * (mi + q.w) * (dwk_i + dwk_j) * r * dloga));
            }
        }
        const double mr = q.w * rinv;
        const double hfc_visc = 0.5 * mr * visc * (dwk_i + dwk_j);
        double hfc = hfc_visc;
        if(hc.DISPH) {
            const double ratio = EVP * inv_iEVP; /* EVP_j / EVP_i */
            hfc += mr * (dwk_i * p_over_rho2_i * ratio + dwk_j * p_over_rho2_j / ratio);
        }
        hfc += mr * (p_over_rho2_i * iDhsml * dwk_i * rr1 + p_over_rho2_j * Dj.x * dwk_j * Dj.y);
        A0 += -hfc * d0;
        A1 += -hfc * d1;
        A2 += -hfc * d2;
        DtE += 0.5 * hfc_visc * vdotr2;
    };

    auto accept = [&](const double r2, const double hj, const int fl) { return r2 > 0 && (r2 < hi2 || r2 < hj * hj) && !(fl & 2); };
    unsigned int dbgc[3] = {0, 0, 0};
    unsigned int nint = 0;
    int fill = 0;
    bool ovf = false;
    if(MODE == 4) {
        HbShared &sh = *reinterpret_cast<HbShared *>(lds);
        nint = heavy_block<true>(a, sh, px, py, pz, hi, accept, pair);
        A0 = hb_sum(A0, sh.red); A1 = hb_sum(A1, sh.red); A2 = hb_sum(A2, sh.red); DtE = hb_sum(DtE, sh.red);
        MaxSig = hb_max(MaxSig, sh.red);
        valid = threadIdx.x == 0;
    } else if(MODE == 3) {
        bool aborted = false;
        nint = heavy_walk<true>(a, lds, px, py, pz, hi, accept, pair, aborted);
        if(aborted) { /* too much for one wave: a whole workgroup takes it */
            if(lane == 0)
                a.heavy2[atomicAdd((unsigned long long *) a.nheavy2, 1ull)] = (int32_t) pi;
            continue;
        }
        A0 = wave_sum(A0); A1 = wave_sum(A1); A2 = wave_sum(A2); DtE = wave_sum(DtE);
        for(int off = 32; off > 0; off >>= 1)
            MaxSig = fmax(MaxSig, __shfl_xor(MaxSig, off));
        valid = lane == 0;
    } else if(MODE != 2)
        nint = ngb_walk<true, MODE == 1, GHOSTS, true>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(true), myl, valid, px, py, pz, hi, accept, pair,
                                                       (MODE == 0 && nint_total && !GHOSTS) ? dbgc : (unsigned int *) nullptr, fill, ovf,
                                                       (GHOSTS && valid) ? qseg[t] : make_int4(-1, -1, -1, -1),
                                                       valid ? pre32_bound(hi, a.Box * 0x1p-20) : 0.f);
    if(MODE == 1) {
        counts[wave * 64 + lane] = ovf ? -1 : fill; /* -1: this target goes to the one-target-per-wave kernel */
        if(ovf)
            nint = 0; /* counted there */
    }
    if(MODE == 2) {
        fill = counts[wave * 64 + lane];
        if(fill < 0) { /* walked on its own (MODE 3) */
            fill = 0;
            valid = false;
        }
        nl_flush(myl, fill, pair);
    }
    if(MODE != 1 && valid) {
        a.hacc[3 * pi] = A0;
        a.hacc[3 * pi + 1] = A1;
        a.hacc[3 * pi + 2] = A2;
        a.dtent[pi] = DtE;
        a.maxsig[pi] = MaxSig;
    }
    unsigned int sn = nint;
    for(int off = 32; off > 0; off >>= 1)
        sn += __shfl_xor(sn, off);
    if(lane == 0 && nint_total)
        atomicAdd(nint_total, (unsigned long long) sn);
    if(MODE == 0 && nint_total && !GHOSTS) { /* diagnostics behind SHQ_SPH_DEBUG: [1] nodes/wave [2] candidates/wave [3] pairs (lanes) [4] flush rounds/wave */
        if(lane == 0) {
            atomicAdd(nint_total + 1, (unsigned long long) dbgc[0]);
            atomicAdd(nint_total + 2, (unsigned long long) dbgc[1]);
            atomicAdd(nint_total + 4, (unsigned long long) dbgc[2]);
        }
    }
    } /* task loop */
}

template <int KT, int MODE, bool GHOSTS = false>
__global__ __launch_bounds__(256, 4) void sph_hydro_kernel(const SphDev a, const int32_t *queue, long long nq, const HydroConst hc,
                                                           unsigned long long *nint_total, int32_t *__restrict__ nlist, long long ntasks,
                                                           int32_t *__restrict__ counts, const long long *d_nq, const int4 *qseg = nullptr)
{
    sph_hydro_body<KT, MODE, GHOSTS>(a, queue, nq, hc, nint_total, nlist, ntasks, counts, d_nq, qseg);
}

/* MODE 4: one target per workgroup of 512 threads */
template <int KT>
__global__ __launch_bounds__(HB_THREADS) void sph_hydro_block_kernel(const SphDev a, const int32_t *queue, const HydroConst hc,
                                                                     unsigned long long *nint_total, const long long *d_nq)
{
    sph_hydro_body<KT, 4, false>(a, queue, 0, hc, nint_total, nullptr, 0, nullptr, d_nq, nullptr);
}

/* HydroOutput::postprocess, hydratree2.hpp:134-148 + winds_decoupled_hydro, winds.h:60-68 */
__global__ void sph_hydro_post_kernel(const SphDev a, const int32_t *queue, long long nq, const double *density,
                                      const double *delay, double hubble_a2, double atime, double WindSpeed, double WindThresh)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nq)
        return;
    const long long i = queue ? (long long) queue[t] : t;
    double de = a.dtent[i];
    de *= SPH_GAMMA_MINUS1 / (hubble_a2 * pow(density[i], SPH_GAMMA_MINUS1));
    if(delay && delay[i] > 0) {
        a.hacc[3 * i] = 0;
        a.hacc[3 * i + 1] = 0;
        a.hacc[3 * i + 2] = 0;
        de = 0;
        double windspeed = WindSpeed * atime;
        const double fac_mu = pow(atime, 3 * (SPH_GAMMA - 1) / 2) / atime;
        windspeed *= fac_mu;
        const double hsml_c = cbrt(WindThresh / density[i]) * atime;
        a.maxsig[i] = hsml_c * fmax(2 * windspeed, a.maxsig[i]);
    }
    a.dtent[i] = de;
}

__global__ void fill_kernel(double *x, long long n, double v)
{
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n)
        x[i] = v;
}

} // namespace

/* ---- host helpers shared with the other operator files (declared in sph_walk.hpp) ------------------------------------ */
int sph_reserve_redo(shq_context *ctx)
{
    const long long n = ctx->numpart;
    const size_t cap = (size_t) (n > 0 ? n : 1);
    SHQ_TRY(ctx->s_numngb.reserve(cap));
    SHQ_TRY(ctx->s_left.reserve(cap));
    SHQ_TRY(ctx->s_right.reserve(cap));
    SHQ_TRY(ctx->s_todo.reserve(cap));
    SHQ_TRY(ctx->s_queue2.reserve(cap));
    SHQ_TRY(ctx->s_queue3.reserve(cap));
    SHQ_TRY(ctx->s_blockcount.reserve(nblk(n) + 1));
    return ctx->s_counters.reserve(8);
}

int sph_reserve_nlist2(shq_context *ctx) { return ctx->s_nlist2.reserve((size_t) NL_REDO_BLOCKS * 4 * NL_ROWS * 64); }

void sph_fill(shq_context *ctx, double *d_x, long long n, double v)
{
    fill_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(d_x, n, v);
}

void sph_gather_leaf_plain(shq_context *ctx, long long nl, double *d_hsml_leaf)
{
    sph_gather_leaf_kernel<<<dim3(nblk(nl)), dim3(256), 0, ctx->stream>>>(nl, ctx->leaf_pidx.ptr, ctx->velp.ptr, nullptr, nullptr, ctx->hsml.ptr, ctx->pflags.ptr,
                                                                         nullptr, ctx->velp_leaf.ptr, nullptr, d_hsml_leaf, ctx->flag_leaf.ptr);
}

int sph_compact_todo(shq_context *ctx, long long size, int32_t *out, long long *newsize)
{
    long long *total = ctx->s_counters.ptr;
    const int nb = (int) nblk(size);
    compact_count_kernel<<<dim3(nb), dim3(256), 0, ctx->stream>>>(ctx->s_todo.ptr, size, ctx->s_blockcount.ptr);
    compact_scan_kernel<<<dim3(1), dim3(1024), 0, ctx->stream>>>(ctx->s_blockcount.ptr, nb, total);
    compact_write_kernel<<<dim3(nb), dim3(256), 0, ctx->stream>>>(ctx->s_todo.ptr, size, ctx->s_blockcount.ptr, out);
    *newsize = 0;
    SHQ_HIP(hipMemcpyAsync(newsize, total, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    return SHQ_OK;
}

int sph_fill_stats(shq_context *ctx, shq_sph_stats *stats, int64_t nq, int niter, const unsigned long long *d_nint, bool hmax_tried)
{
    unsigned long long h_c[3] = {0, 0, 0}; /* [0] interactions, [2] bits of the largest Hsml tried (density only) */
    SHQ_HIP(hipMemcpyAsync(h_c, d_nint, hmax_tried ? sizeof(h_c) : sizeof(h_c[0]), hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    (void) hipEventElapsedTime(&ms, ctx->ev_begin[SHQ_T_SPH], ctx->ev_end[SHQ_T_SPH]);
    stats->ntargets = nq;
    stats->ninteractions = (int64_t) h_c[0];
    stats->niterations = niter;
    stats->kernel_ms = ms;
    memcpy(&stats->hsml_max_tried, &h_c[2], sizeof(double));
    return SHQ_OK;
}

/* Prepass + leaf gather: fills velp (and hydC/hydD when hp != NULL) and their leaf-order copies. */
int shq_sph_prepare(shq_context *ctx, const shq_kick_factors *kf, const shq_hydro_params *hp, const double *d_evp_in)
{
    const long long n = ctx->numpart;
    SHQ_TRY(ctx->velp.reserve(n > 0 ? n : 1));
    SHQ_TRY(ctx->hydC.reserve(n > 0 ? n : 1));
    SHQ_TRY(ctx->hydD.reserve(n > 0 ? n : 1));
    const long long nl = ctx->ntreeparts + SHQ_NMAXCHILD;
    SHQ_CHECK(nl < (1ll << 30), SHQ_ERR_INVALID, "SPH walk: more than 2^30 leaf slots (the candidate tile keeps two flag bits on top of the slot)");
    SHQ_TRY(ctx->velp_leaf.reserve(nl));
    SHQ_TRY(ctx->hydrec_leaf.reserve(nl * sizeof(HydRec) + 128));
    SHQ_TRY(ctx->hsml_leaf.reserve(nl));
    SHQ_TRY(ctx->flag_leaf.reserve(nl));
    SHQ_TRY(ctx->posf_leaf.reserve(nl));
    SHQ_TRY(ctx->ngarb_leaf.reserve(nl));
    if(n == 0)
        return SHQ_OK;
    PredArgs a;
    a.n = n;
    a.pflags = ctx->pflags.ptr;
    a.vel = ctx->vel.ptr;
    a.treeacc = ctx->treeacc.ptr;
    a.gravpm = ctx->gravpm.ptr;
    a.hydroaccel = ctx->g_hydroaccel.ptr;
    a.bin_grav = ctx->bin_grav.ptr;
    a.bin_hydro = ctx->bin_hydro.ptr;
    a.entropy = ctx->g_entropy.ptr;
    a.dtentropy = ctx->g_dtentropy.ptr;
    a.hsml = ctx->hsml.ptr;
    a.density = ctx->g_density.ptr;
    a.egywt = ctx->g_egywt.ptr;
    a.dhsmlegy = ctx->g_dhsmlegy.ptr;
    a.divvel = ctx->g_divvel.ptr;
    a.curlvel = ctx->g_curlvel.ptr;
    a.velp = ctx->velp.ptr;
    a.hydC = ctx->hydC.ptr;
    a.hydD = ctx->hydD.ptr;
    a.evp_in = d_evp_in;
    a.kf = *kf;
    a.hydro = hp ? 1 : 0;
    a.DISPH = hp ? hp->DensityIndependentSphOn : 0;
    a.fac_mu = hp ? hp->fac_mu : 1;
    a.contrast = hp ? hp->DensityContrastLimit : 0;
    for(int i = 0; i <= SHQ_TIMEBINS; i++)
        a.drifts[i] = hp ? hp->drifts[i] : 0;
    sph_predict_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(a);
    sph_gather_leaf_kernel<<<dim3(nblk(nl)), dim3(256), 0, ctx->stream>>>(
        nl, ctx->leaf_pidx.ptr, ctx->velp.ptr, hp ? ctx->hydC.ptr : nullptr, hp ? ctx->hydD.ptr : nullptr, ctx->hsml.ptr,
        ctx->pflags.ptr, ctx->g_delaytime.ptr, ctx->velp_leaf.ptr, hp ? reinterpret_cast<HydRec *>(ctx->hydrec_leaf.ptr) : nullptr,
        ctx->hsml_leaf.ptr, ctx->flag_leaf.ptr, ctx->posm_leaf.ptr, ctx->posf_leaf.ptr, ldexp(ctx->treeBox, -20));
    if(ctx->numnodes > 0)
        sph_leaf_ngarb_kernel<<<dim3(nblk(ctx->numnodes)), dim3(256), 0, ctx->stream>>>((int) ctx->numnodes, ctx->nodeC.ptr, ctx->flag_leaf.ptr,
                                                                                      ctx->ngarb_leaf.ptr);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* ---- launch: two kernels per chunk of targets + redo of overflowed waves ---------------------------- */
#define NL_CHUNK (1ll << 22)  /* targets per chunk: 4 Mi x NL_CAP x 4 B = 4 GB of list scratch */
#define NL_BLOCK_BLOCKS 512  /* 512-thread workgroups of the one-target-per-workgroup kernel */
#define NL_HEAVY_BLOCKS 8192 /* single-wave workgroups of the one-target-per-wave kernel (it takes its queue length from the device) */

/* targets of the chunk whose lists overflowed: append them to the queue of the one-target-per-wave kernel */
__global__ void sph_collect_redo_kernel(const int32_t *__restrict__ counts, const int32_t *__restrict__ queue, long long nq, int32_t *redo,
                                        long long *nredo)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nq || counts[t] >= 0)
        return;
    const long long at = (long long) atomicAdd((unsigned long long *) nredo, 1ull);
    redo[at] = queue ? queue[t] : (int32_t) t;
}

static long long nl_chunk_waves(long long nq)
{
    const long long chunk = nq < NL_CHUNK ? nq : NL_CHUNK;
    return ((chunk + 255) / 256) * 4;
}

/* Walk and evaluation in a pipeline (round 4).  The walk kernel is bound by the vector and scalar pipes (tools/sph_ab.sh with the
 * SPH_PROBE builds: 3.2 ms of node tests + 1.5 ms of candidate tests for the 128^3 hydro pass), the evaluation kernel by the texture
 * addresser (eight to ten 16-byte gathers per pair from 64 different lines, 37 % VALU busy): with the targets cut into NL_PIPE pieces, the
 * evaluation of piece k runs on a second stream beside the walk of piece k + 1, two list regions in turn.  SHQ_SPH_PIPE=0: one after the
 * other, as before (the same lists, the same sums). */
#define NL_PIPE 4
#define NL_PIPE_MIN (1ll << 19)
static bool nl_pipelined(const int32_t *q, long long nq)
{
    static const bool on = getenv("SHQ_SPH_PIPE") && atoi(getenv("SHQ_SPH_PIPE")) != 0;
    return on && q != nullptr && nq > NL_PIPE_MIN;
}
static long long nl_pipe_targets(long long nq)
{
    const long long c = (((nq + NL_PIPE - 1) / NL_PIPE) + 255) / 256 * 256;
    return c < NL_CHUNK ? c : NL_CHUNK;
}

/* list scratch: one region per wave of a chunk (both layouts fit: two pieces of a quarter each, or the whole), followed by one per
 * wave of the fused redo kernel */
static int reserve_nlist(shq_context *ctx, long long nq)
{
    const long long waves = nl_chunk_waves(nq) + NL_REDO_BLOCKS * 4;
    SHQ_TRY(ctx->s_nlist.reserve((size_t) waves * NL_ROWS * 64));
    SHQ_TRY(ctx->s_ncount.reserve((size_t) (nl_chunk_waves(nq) + 8) * 64));
    SHQ_TRY(ctx->s_redo.reserve((size_t) (nq > 0 ? nq : 1)));
    SHQ_TRY(ctx->s_redo2.reserve((size_t) (nq > 0 ? nq : 1)));
    for(int i = 0; i < 4; i++)
        if(!ctx->ev_sph[i])
            SHQ_HIP(hipEventCreateWithFlags(&ctx->ev_sph[i], hipEventDisableTiming));
    return SHQ_OK;
}

/* Runs walk<1> and eval<2> over [q, q + nq) in chunks, then the one-target-per-wave kernel <3> over the targets whose
 * lists overflowed (their number is only known on the device: the kernel reads it there). */
template <class LaunchW, class LaunchP, class LaunchF, class LaunchB>
static int launch_two_kernel(shq_context *ctx, const int32_t *q, long long nq, long long nq_reserved, LaunchW &&walk, LaunchP &&eval,
                             LaunchF &&fused, LaunchB &&block)
{
    long long *d_nredo = ctx->s_counters.ptr + 6;
    SHQ_HIP(hipMemsetAsync(d_nredo, 0, 2 * sizeof(long long), ctx->stream)); /* [6] targets for a wave of their own, [7] for a workgroup */
    int32_t *lists = ctx->s_nlist.ptr;
    int32_t *fused_lists = ctx->s_nlist.ptr + (size_t) nl_chunk_waves(nq_reserved) * NL_ROWS * 64;
    SHQ_CHECK(q || nq <= NL_CHUNK, SHQ_ERR_INVALID, "SPH walk: more than %lld targets need an explicit queue", (long long) NL_CHUNK);
    const bool pipe = nl_pipelined(q, nq) && ctx->stream_pair;
    const long long chunk = pipe ? nl_pipe_targets(nq) : NL_CHUNK;
    /* pipelined: two regions of a piece's waves each (a piece is at most a quarter of what was reserved, rounded up to 256 targets) */
    const size_t region = pipe ? (size_t) ((chunk + 255) / 256 * 4) * NL_ROWS * 64 : 0;
    const size_t cregion = pipe ? (size_t) ((chunk + 255) / 256 * 4 + 4) * 64 : 0;
    static const bool hi = getenv("SHQ_SPH_PIPE") && atoi(getenv("SHQ_SPH_PIPE")) == 2; /* the evaluation on the high-priority stream */
    hipStream_t sw = ctx->stream, se = pipe ? (hi && ctx->stream_pm ? ctx->stream_pm : ctx->stream_pair) : ctx->stream;
    int k = 0;
    for(long long off = 0; off < nq; off += chunk, k++) {
        const long long m = (nq - off < chunk) ? nq - off : chunk;
        const long long ntasks = (m + 255) / 256;
        const int32_t *qc = q ? q + off : nullptr;
        const long long wtasks = (m + 64 * SPH_WALK_WPB - 1) / (64 * SPH_WALK_WPB);
        const int b = k & 1;
        int32_t *lb = lists + b * region, *cb = ctx->s_ncount.ptr + b * cregion;
        if(pipe && k >= 2)
            SHQ_HIP(hipStreamWaitEvent(sw, ctx->ev_sph[2 + b], 0)); /* the evaluation of piece k - 2 is done with this region */
        walk(sw, (unsigned) wtasks, qc, m, wtasks, lb, cb);
        if(pipe) {
            SHQ_HIP(hipEventRecord(ctx->ev_sph[b], sw));
            SHQ_HIP(hipStreamWaitEvent(se, ctx->ev_sph[b], 0));
        }
        eval(se, (unsigned) ntasks, qc, m, ntasks, lb, cb);
        sph_collect_redo_kernel<<<dim3(nblk(m)), dim3(256), 0, se>>>(cb, qc, m, ctx->s_redo.ptr, d_nredo);
        if(pipe)
            SHQ_HIP(hipEventRecord(ctx->ev_sph[2 + b], se));
    }
    if(pipe)
        for(int b = 0; b < 2 && b < k; b++)
            SHQ_HIP(hipStreamWaitEvent(sw, ctx->ev_sph[2 + b], 0));
    fused((unsigned) NL_HEAVY_BLOCKS, ctx->s_redo.ptr, fused_lists, d_nredo);
    block((unsigned) NL_BLOCK_BLOCKS, ctx->s_redo2.ptr, d_nredo + 1);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

template <int KT>
static int launch_density(shq_context *ctx, const SphDev &a, const int32_t *q, long long nq, long long nq_reserved, int wd,
                          unsigned long long *nint)
{
    hipStream_t st = ctx->stream;
    return launch_two_kernel(
        ctx, q, nq, nq_reserved,
        [&](hipStream_t s, unsigned grid, const int32_t *qc, long long m, long long ntasks, int32_t *lists, int32_t *counts) {
            sph_density_kernel<KT, 1><<<dim3(grid), dim3(64 * SPH_WALK_WPB), 0, s>>>(a, qc, m, wd, nint, lists, ntasks, counts, nullptr);
        },
        [&](hipStream_t s, unsigned grid, const int32_t *qc, long long m, long long ntasks, int32_t *lists, int32_t *counts) {
            sph_density_kernel<KT, 2><<<dim3(grid), dim3(256), 0, s>>>(a, qc, m, wd, nint, lists, ntasks, counts, nullptr);
        },
        [&](unsigned grid, const int32_t *redo, int32_t *lists, const long long *d_nredo) {
            sph_density_kernel<KT, 3><<<dim3(grid), dim3(64), 0, st>>>(a, redo, 0, wd, nint, lists, 0, nullptr, d_nredo);
        },
        [&](unsigned grid, const int32_t *redo2, const long long *d_n2) {
            sph_density_block_kernel<KT><<<dim3(grid), dim3(HB_THREADS), 0, st>>>(a, redo2, wd, nint, d_n2);
        });
}
template <int KT>
static int launch_hydro(shq_context *ctx, const SphDev &a, const int32_t *q, long long nq, const HydroConst &hc, unsigned long long *nint)
{
    hipStream_t st = ctx->stream;
    return launch_two_kernel(
        ctx, q, nq, nq,
        [&](hipStream_t s, unsigned grid, const int32_t *qc, long long m, long long ntasks, int32_t *lists, int32_t *counts) {
            sph_hydro_kernel<KT, 1><<<dim3(grid), dim3(64 * SPH_WALK_WPB), 0, s>>>(a, qc, m, hc, nint, lists, ntasks, counts, nullptr);
        },
        [&](hipStream_t s, unsigned grid, const int32_t *qc, long long m, long long ntasks, int32_t *lists, int32_t *counts) {
            sph_hydro_kernel<KT, 2><<<dim3(grid), dim3(256), 0, s>>>(a, qc, m, hc, nint, lists, ntasks, counts, nullptr);
        },
        [&](unsigned grid, const int32_t *redo, int32_t *lists, const long long *d_nredo) {
            sph_hydro_kernel<KT, 3><<<dim3(grid), dim3(64), 0, st>>>(a, redo, 0, hc, nint, lists, 0, nullptr, d_nredo);
        },
        [&](unsigned grid, const int32_t *redo2, const long long *d_n2) {
            sph_hydro_block_kernel<KT><<<dim3(grid), dim3(HB_THREADS), 0, st>>>(a, redo2, hc, nint, d_n2);
        });
}

/* Device-resident density(): queue = d_queue[0..nq) of particle indices (already filtered by
 * DensityQuery::haswork).  Runs the whole Hsml loop. */
/* ---- density in phases: the set of hooks a TreeWalk backend overrides (treewalk2.cuh:212-394) --------------------
 * begin (DensityOutput ctor) -> { primary (ev_primary) -> [reduce of returned export results] -> post (ev_postprocess +
 * the do_hsml_loop bookkeeping, treewalk2.h:480-557) } until the redo queue is empty -> end. */
static SphDev density_dev(shq_context *ctx)
{
    SphDev a = make_dev(ctx, ctx->sphrun.dp.BoxSize);
    a.gradrho = ctx->sphrun.want_gradrho ? ctx->s_gradrho.ptr : nullptr;
    return a;
}

int shq_sph_density_begin(shq_context *ctx, const shq_density_params *p, const int32_t *d_queue, int64_t nq, int want_gradrho)
{
    const long long n = ctx->numpart;
    const size_t cap = (size_t) (n > 0 ? n : 1);
    SHQ_TRY(sph_reserve_redo(ctx));
    SHQ_TRY(ctx->s_dhsmldens.reserve(cap));
    SHQ_TRY(ctx->s_rot.reserve(3 * cap));
    SHQ_TRY(reserve_nlist(ctx, nq));
    if(want_gradrho)
        SHQ_TRY(ctx->s_gradrho.reserve(3 * cap));
    SHQ_CHECK(p->DensityKernelType == 1 || p->DensityKernelType == 2 || p->DensityKernelType == 4, SHQ_ERR_INVALID,
              "unknown DensityKernelType %d", p->DensityKernelType);
    /* DensityOutput ctor, densitytree2.hpp:92-98 */
    if(n > 0) {
        SHQ_HIP(hipMemsetAsync(ctx->s_left.ptr, 0, sizeof(double) * n, ctx->stream));
        SHQ_HIP(hipMemsetAsync(ctx->s_numngb.ptr, 0, sizeof(double) * n, ctx->stream));
        sph_fill(ctx, ctx->s_right.ptr, n, p->BoxSize);
    }
    SHQ_HIP(hipMemsetAsync(ctx->s_counters.ptr, 0, sizeof(long long) * 8, ctx->stream));
    shq_context::SphRun &r = ctx->sphrun;
    r.dp = *p;
    r.want_gradrho = want_gradrho;
    r.cur = d_queue;
    r.size = nq;
    r.nq0 = nq;
    r.wsel = 0;
    r.niter = 0;
    r.phase = 1;
    SHQ_HIP(hipEventRecord(ctx->ev_begin[SHQ_T_SPH], ctx->stream));
    return SHQ_OK;
}

int shq_sph_density_primary(shq_context *ctx)
{
    shq_context::SphRun &r = ctx->sphrun;
    SHQ_CHECK(r.phase == 1, SHQ_ERR_STATE, "density primary: no density walk is open");
    if(r.size == 0)
        return SHQ_OK;
    const SphDev a = density_dev(ctx);
    unsigned long long *nint = reinterpret_cast<unsigned long long *>(ctx->s_counters.ptr + 1);
    switch(r.dp.DensityKernelType) {
    case 1: SHQ_TRY(launch_density<1>(ctx, a, r.cur, r.size, r.nq0, r.dp.WindsDecouple, nint)); break;
    case 2: SHQ_TRY(launch_density<2>(ctx, a, r.cur, r.size, r.nq0, r.dp.WindsDecouple, nint)); break;
    default: SHQ_TRY(launch_density<4>(ctx, a, r.cur, r.size, r.nq0, r.dp.WindsDecouple, nint)); break;
    }
    return SHQ_OK;
}

int shq_sph_density_post(shq_context *ctx, int64_t *nredo)
{
    shq_context::SphRun &r = ctx->sphrun;
    SHQ_CHECK(r.phase == 1, SHQ_ERR_STATE, "density postprocess: no density walk is open");
    const shq_density_params *p = &r.dp;
    *nredo = 0;
    if(r.size > 0) {
        const SphDev a = density_dev(ctx);
        PostArgs pa;
        pa.Box = p->BoxSize;
        pa.DesNumNgb = p->DesNumNgb;
        pa.DesNumNgbBH = p->DesNumNgbBH;
        pa.MinGasHsml = p->MinGasHsml;
        pa.MaxDev = p->MaxNumNgbDeviation;
        pa.update_hsml = p->update_hsml;
        pa.BlackHoleOn = p->BlackHoleOn;
        pa.DoEgyDensity = p->DoEgyDensity;
        pa.hmax_tried = reinterpret_cast<unsigned long long *>(ctx->s_counters.ptr + 3);
        sph_density_post_kernel<<<dim3(nblk(r.size)), dim3(256), 0, ctx->stream>>>(a, r.cur, r.size, pa, ctx->s_todo.ptr);
        SHQ_HIP(hipGetLastError());
    }
    r.niter++;
    if(!p->update_hsml || r.size == 0) {
        r.size = 0;
        return SHQ_OK;
    }
    int32_t *bufs[2] = {ctx->s_queue2.ptr, ctx->s_queue3.ptr};
    long long newsize = 0;
    SHQ_TRY(sph_compact_todo(ctx, r.size, bufs[r.wsel], &newsize));
    r.size = newsize;
    if(newsize == 0)
        return SHQ_OK;
    /* the neighbours' Hsml copy in leaf order is only read by hydro, so no refresh is needed here */
    r.cur = bufs[r.wsel];
    r.wsel ^= 1;
    if(r.niter > SPH_MAXITER) {
        shq_set_error("failed to converge density for %lld particles", newsize);
        return SHQ_ERR_NOCONV;
    }
    *nredo = newsize;
    return SHQ_OK;
}

int shq_sph_density_end(shq_context *ctx, shq_sph_stats *stats)
{
    shq_context::SphRun &r = ctx->sphrun;
    SHQ_CHECK(r.phase == 1, SHQ_ERR_STATE, "density end: no density walk is open");
    r.phase = 0;
    SHQ_HIP(hipEventRecord(ctx->ev_end[SHQ_T_SPH], ctx->stream));
    if(stats)
        SHQ_TRY(sph_fill_stats(ctx, stats, r.nq0, r.niter, reinterpret_cast<unsigned long long *>(ctx->s_counters.ptr + 1), true));
    return SHQ_OK;
}

int shq_sph_density_device(shq_context *ctx, const shq_density_params *p, const int32_t *d_queue, int64_t nq, int want_gradrho,
                           shq_sph_stats *stats)
{
    SHQ_TRY(shq_sph_density_begin(ctx, p, d_queue, nq, want_gradrho));
    int64_t nredo = 0;
    do {
        SHQ_TRY(shq_sph_density_primary(ctx));
        SHQ_TRY(shq_sph_density_post(ctx, &nredo));
    } while(nredo > 0);
    return shq_sph_density_end(ctx, stats);
}

/* DensityResult::reduce<TREEWALK_GHOSTS> (densitytree2.hpp:308-343): one thread per table entry, the first entry of
 * a run of equal places adds the run in order (entries arrive grouped by target). */
__global__ void sph_density_reduce_kernel(const SphDev a, long long n, const int32_t *__restrict__ place, const shq_density_result *__restrict__ res)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    const long long i = place[k];
    if(k > 0 && place[k - 1] == i)
        return;
    const int type = a.pflags[i] >> 4;
    for(long long j = k; j < n && place[j] == i; j++) {
        const shq_density_result r = res[j];
        a.numngb[i] += r.Ngb;
        a.dhsmldens[i] += r.DhsmlDensity;
        if(type == 0 || type == 5) {
            a.rho[i] += r.Rho;
            a.div[i] += r.Div;
        }
        if(type == 0) {
            a.rot[3 * i] += r.Rot[0];
            a.rot[3 * i + 1] += r.Rot[1];
            a.rot[3 * i + 2] += r.Rot[2];
            if(a.gradrho) {
                a.gradrho[3 * i] += r.GradRho[0];
                a.gradrho[3 * i + 1] += r.GradRho[1];
                a.gradrho[3 * i + 2] += r.GradRho[2];
            }
            a.egyrho[i] += r.EgyRho;
            a.dhsmlegy[i] += r.DhsmlEgyDensity;
        }
    }
}

int shq_sph_density_reduce(shq_context *ctx, const int32_t *d_place, const void *d_results, int64_t n)
{
    SHQ_CHECK(ctx->sphrun.phase == 1, SHQ_ERR_STATE, "density reduce: no density walk is open");
    if(n == 0)
        return SHQ_OK;
    const SphDev a = density_dev(ctx);
    sph_density_reduce_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(a, n, d_place, static_cast<const shq_density_result *>(d_results));
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* LocalNgbTreeWalk::visit<TREEWALK_GHOSTS> for imported DensityQuery records: the target-side arrays of the
 * walk kernel are swapped for query-indexed ones, the neighbour side stays the local tree.  d_q* are nq long;
 * d_out holds 12 nq doubles: Ngb, DhsmlDensity, Rho, Div, EgyRho, DhsmlEgyDensity, Rot[3], GradRho[3] (SoA). */
int shq_sph_density_secondary(shq_context *ctx, const shq_density_params *p, const double4 *d_qposm, const double *d_qhsml,
                              const double4 *d_qvelp, const uint8_t *d_qflags, const int4 *d_qseg, int64_t nq, double *d_out,
                              unsigned long long *d_nint)
{
    if(nq == 0)
        return SHQ_OK;
    SHQ_CHECK(p->DensityKernelType == 1 || p->DensityKernelType == 2 || p->DensityKernelType == 4, SHQ_ERR_INVALID,
              "unknown DensityKernelType %d", p->DensityKernelType);
    SHQ_TRY(sph_reserve_nlist2(ctx));
    SphDev a = make_dev(ctx, p->BoxSize);
    a.posm = d_qposm;
    a.hsml = const_cast<double *>(d_qhsml);
    a.velp = d_qvelp;
    a.pflags = d_qflags;
    a.numngb = d_out;
    a.dhsmldens = d_out + nq;
    a.rho = d_out + 2 * nq;
    a.div = d_out + 3 * nq;
    a.egyrho = d_out + 4 * nq;
    a.dhsmlegy = d_out + 5 * nq;
    a.rot = d_out + 6 * nq;
    a.gradrho = d_out + 9 * nq;
    const long long ntasks = (nq + 255) / 256;
    const unsigned grid = (unsigned) (ntasks < NL_REDO_BLOCKS ? ntasks : NL_REDO_BLOCKS);
    hipStream_t st = ctx->stream;
    switch(p->DensityKernelType) {
    case 1: sph_density_kernel<1, 0, true><<<dim3(grid), dim3(256), 0, st>>>(a, nullptr, nq, p->WindsDecouple, d_nint, ctx->s_nlist2.ptr, ntasks, nullptr, nullptr, d_qseg); break;
    case 2: sph_density_kernel<2, 0, true><<<dim3(grid), dim3(256), 0, st>>>(a, nullptr, nq, p->WindsDecouple, d_nint, ctx->s_nlist2.ptr, ntasks, nullptr, nullptr, d_qseg); break;
    default: sph_density_kernel<4, 0, true><<<dim3(grid), dim3(256), 0, st>>>(a, nullptr, nq, p->WindsDecouple, d_nint, ctx->s_nlist2.ptr, ntasks, nullptr, nullptr, d_qseg); break;
    }
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* ---- hydro in phases: begin -> primary (ev_primary) -> [reduce of returned export results] -> post (ev_postprocess) -> end */
static HydroConst hydro_const(const shq_hydro_params *p)
{
    HydroConst hc;
    hc.hubble_a2 = p->hubble_a2;
    hc.fac_mu = p->fac_mu;
    hc.fac_vsic_fix = p->fac_vsic_fix;
    hc.ArtBulkViscConst = p->ArtBulkViscConst;
    hc.contrast = p->DensityContrastLimit;
    hc.DISPH = p->DensityIndependentSphOn;
    return hc;
}

int shq_sph_hydro_begin(shq_context *ctx, const shq_hydro_params *p, const int32_t *d_queue, int64_t nq)
{
    const long long n = ctx->numpart;
    const size_t cap = (size_t) (n > 0 ? n : 1);
    SHQ_TRY(ctx->g_hydroaccel_out.reserve(3 * cap));
    SHQ_TRY(ctx->g_dtentropy_out.reserve(cap));
    SHQ_TRY(ctx->g_maxsignalvel.reserve(cap));
    SHQ_TRY(ctx->s_counters.reserve(8));
    SHQ_TRY(reserve_nlist(ctx, nq));
    SHQ_CHECK(p->DensityKernelType == 1 || p->DensityKernelType == 2 || p->DensityKernelType == 4, SHQ_ERR_INVALID,
              "unknown DensityKernelType %d", p->DensityKernelType);
    SHQ_HIP(hipMemsetAsync(ctx->s_counters.ptr, 0, sizeof(long long) * 8, ctx->stream));
    shq_context::SphRun &r = ctx->sphrun;
    r.hp = *p;
    r.cur = d_queue;
    r.size = nq;
    r.nq0 = nq;
    r.niter = 0;
    r.phase = 2;
    SHQ_HIP(hipEventRecord(ctx->ev_begin[SHQ_T_SPH], ctx->stream));
    return SHQ_OK;
}

int shq_sph_hydro_primary(shq_context *ctx)
{
    shq_context::SphRun &r = ctx->sphrun;
    SHQ_CHECK(r.phase == 2, SHQ_ERR_STATE, "hydro primary: no hydro walk is open");
    if(r.size == 0)
        return SHQ_OK;
    const SphDev a = make_dev(ctx, r.hp.BoxSize);
    const HydroConst hc = hydro_const(&r.hp);
    unsigned long long *nint = reinterpret_cast<unsigned long long *>(ctx->s_counters.ptr + 1);
    switch(r.hp.DensityKernelType) {
    case 1: SHQ_TRY(launch_hydro<1>(ctx, a, r.cur, r.size, hc, nint)); break;
    case 2: SHQ_TRY(launch_hydro<2>(ctx, a, r.cur, r.size, hc, nint)); break;
    default: SHQ_TRY(launch_hydro<4>(ctx, a, r.cur, r.size, hc, nint)); break;
    }
    return SHQ_OK;
}

int shq_sph_hydro_post(shq_context *ctx)
{
    shq_context::SphRun &r = ctx->sphrun;
    SHQ_CHECK(r.phase == 2, SHQ_ERR_STATE, "hydro postprocess: no hydro walk is open");
    if(r.size > 0) {
        const SphDev a = make_dev(ctx, r.hp.BoxSize);
        const shq_hydro_params *p = &r.hp;
        sph_hydro_post_kernel<<<dim3(nblk(r.size)), dim3(256), 0, ctx->stream>>>(a, r.cur, r.size, ctx->g_density.ptr, ctx->g_delaytime.ptr,
                                                                                p->hubble_a2, p->atime, p->WindSpeed, p->WindFreeTravelDensThresh);
        SHQ_HIP(hipGetLastError());
    }
    r.niter = 1;
    return SHQ_OK;
}

int shq_sph_hydro_end(shq_context *ctx, shq_sph_stats *stats)
{
    shq_context::SphRun &r = ctx->sphrun;
    SHQ_CHECK(r.phase == 2, SHQ_ERR_STATE, "hydro end: no hydro walk is open");
    r.phase = 0;
    SHQ_HIP(hipEventRecord(ctx->ev_end[SHQ_T_SPH], ctx->stream));
    if(stats) {
        unsigned long long *nint = reinterpret_cast<unsigned long long *>(ctx->s_counters.ptr + 1);
        SHQ_TRY(sph_fill_stats(ctx, stats, r.nq0, 1, nint));
        if(getenv("SHQ_SPH_DEBUG") && r.nq0 > 0) {
            unsigned long long d[5];
            SHQ_HIP(hipMemcpy(d, nint, sizeof(d), hipMemcpyDeviceToHost));
            const double nw = (double) ((r.nq0 + 63) / 64);
            fprintf(stderr, "[shq] hydro per wave: nodes %.1f candidates %.1f pair rounds %.1f; per target: candidates %.1f\n",
                    d[1] / nw, d[2] / nw, d[4] / nw, (double) d[0] / r.nq0);
        }
    }
    return SHQ_OK;
}

int shq_sph_hydro_device(shq_context *ctx, const shq_hydro_params *p, const int32_t *d_queue, int64_t nq, shq_sph_stats *stats)
{
    SHQ_TRY(shq_sph_hydro_begin(ctx, p, d_queue, nq));
    SHQ_TRY(shq_sph_hydro_primary(ctx));
    SHQ_TRY(shq_sph_hydro_post(ctx));
    return shq_sph_hydro_end(ctx, stats);
}

/* HydroResult::reduce<TREEWALK_GHOSTS>, hydratree2.hpp:213-227 */
__global__ void sph_hydro_reduce_kernel(const SphDev a, long long n, const int32_t *__restrict__ place, const shq_hydro_result *__restrict__ res)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    const long long i = place[k];
    if(k > 0 && place[k - 1] == i)
        return;
    double a0 = a.hacc[3 * i], a1 = a.hacc[3 * i + 1], a2 = a.hacc[3 * i + 2], de = a.dtent[i], ms = a.maxsig[i];
    for(long long j = k; j < n && place[j] == i; j++) {
        const shq_hydro_result r = res[j];
        a0 += r.Acc[0];
        a1 += r.Acc[1];
        a2 += r.Acc[2];
        de += r.DtEntropy;
        if(ms < r.MaxSignalVel)
            ms = r.MaxSignalVel;
    }
    a.hacc[3 * i] = a0;
    a.hacc[3 * i + 1] = a1;
    a.hacc[3 * i + 2] = a2;
    a.dtent[i] = de;
    a.maxsig[i] = ms;
}

int shq_sph_hydro_reduce(shq_context *ctx, const int32_t *d_place, const void *d_results, int64_t n)
{
    SHQ_CHECK(ctx->sphrun.phase == 2, SHQ_ERR_STATE, "hydro reduce: no hydro walk is open");
    if(n == 0)
        return SHQ_OK;
    const SphDev a = make_dev(ctx, ctx->sphrun.hp.BoxSize);
    sph_hydro_reduce_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(a, n, d_place, static_cast<const shq_hydro_result *>(d_results));
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* visit<TREEWALK_GHOSTS> for imported HydroQuery records; d_out: 5 nq doubles, Acc[3] (AoS, 3 nq), DtEntropy, MaxSignalVel */
int shq_sph_hydro_secondary(shq_context *ctx, const shq_hydro_params *p, const double4 *d_qposm, const double *d_qhsml,
                            const double4 *d_qvelp, const double4 *d_qC, const double4 *d_qD, const int4 *d_qseg, int64_t nq, double *d_out,
                            unsigned long long *d_nint)
{
    if(nq == 0)
        return SHQ_OK;
    SHQ_CHECK(p->DensityKernelType == 1 || p->DensityKernelType == 2 || p->DensityKernelType == 4, SHQ_ERR_INVALID,
              "unknown DensityKernelType %d", p->DensityKernelType);
    SHQ_TRY(sph_reserve_nlist2(ctx));
    SphDev a = make_dev(ctx, p->BoxSize);
    a.posm = d_qposm;
    a.hsml = const_cast<double *>(d_qhsml);
    a.velp = d_qvelp;
    a.hydC = d_qC;
    a.hydD = d_qD;
    a.hacc = d_out;
    a.dtent = d_out + 3 * nq;
    a.maxsig = d_out + 4 * nq;
    const HydroConst hc = hydro_const(p);
    const long long ntasks = (nq + 255) / 256;
    const unsigned grid = (unsigned) (ntasks < NL_REDO_BLOCKS ? ntasks : NL_REDO_BLOCKS);
    hipStream_t st = ctx->stream;
    switch(p->DensityKernelType) {
    case 1: sph_hydro_kernel<1, 0, true><<<dim3(grid), dim3(256), 0, st>>>(a, nullptr, nq, hc, d_nint, ctx->s_nlist2.ptr, ntasks, nullptr, nullptr, d_qseg); break;
    case 2: sph_hydro_kernel<2, 0, true><<<dim3(grid), dim3(256), 0, st>>>(a, nullptr, nq, hc, d_nint, ctx->s_nlist2.ptr, ntasks, nullptr, nullptr, d_qseg); break;
    default: sph_hydro_kernel<4, 0, true><<<dim3(grid), dim3(256), 0, st>>>(a, nullptr, nq, hc, d_nint, ctx->s_nlist2.ptr, ntasks, nullptr, nullptr, d_qseg); break;
    }
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* The export queries of a walk in progress, one record per table entry (DensityQuery / HydroQuery ctors,
 * densitytree2.hpp:267-278, hydratree2.hpp:165-191): everything comes from the resident arrays. */
__global__ void sph_fill_density_queries_kernel(const SphDev a, long long n, const shq_data_index *__restrict__ table, shq_density_query *out)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    const shq_data_index e = table[k];
    const long long i = e.Index;
    shq_density_query q;
    const double4 p = a.posm[i], v = a.velp[i];
    q.Pos[0] = p.x; q.Pos[1] = p.y; q.Pos[2] = p.z;
    for(int j = 0; j < 4; j++)
        q.NodeList[j] = e.NodeList[j];
    q.Vel[0] = v.x; q.Vel[1] = v.y; q.Vel[2] = v.z;
    q.Hsml = a.hsml[i];
    q.Type = a.pflags[i] >> 4;
    q.pad_ = 0;
    out[k] = q;
}

__global__ void sph_fill_hydro_queries_kernel(const SphDev a, long long n, const shq_data_index *__restrict__ table, const double *__restrict__ density,
                                              const uint8_t *__restrict__ bin_hydro, int DISPH, double fac_mu, shq_hydro_query *out)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    const shq_data_index e = table[k];
    const long long i = e.Index;
    shq_hydro_query q;
    const double4 p = a.posm[i], v = a.velp[i];
    q.Pos[0] = p.x; q.Pos[1] = p.y; q.Pos[2] = p.z;
    for(int j = 0; j < 4; j++)
        q.NodeList[j] = e.NodeList[j];
    const double eom = DISPH ? a.egyrho[i] : density[i]; /* SPH_EOMDensity, hydratree2.hpp:36-45 */
    q.EgyRho = eom;
    q.EntVarPred = v.w;
    q.Vel[0] = v.x; q.Vel[1] = v.y; q.Vel[2] = v.z;
    q.Hsml = a.hsml[i];
    q.Mass = p.w;
    q.Density = density[i];
    q.Pressure = pressure_predict(eom, v.w);
    q.SPH_DhsmlDensityFactor = a.dhsmlegy[i];
    const double cs = sqrt(SPH_GAMMA * q.Pressure / eom);
    q.F1 = fabs(a.div[i]) / (fabs(a.div[i]) + a.curl[i] + 0.0001 * cs / q.Hsml / fac_mu);
    q.TimeBinHydro = bin_hydro[i];
    q.pad_ = 0;
    out[k] = q;
}

int shq_sph_fill_queries_device(shq_context *ctx, const shq_data_index *d_table, int64_t n, void *d_out)
{
    const shq_context::SphRun &r = ctx->sphrun;
    SHQ_CHECK(r.phase == 1 || r.phase == 2, SHQ_ERR_STATE, "fill_queries: no SPH walk is open");
    if(n == 0)
        return SHQ_OK;
    const SphDev a = make_dev(ctx, ctx->treeBox);
    if(r.phase == 1)
        sph_fill_density_queries_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(a, n, d_table, static_cast<shq_density_query *>(d_out));
    else
        sph_fill_hydro_queries_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(a, n, d_table, ctx->g_density.ptr, ctx->bin_hydro.ptr,
                                                                                   r.hp.DensityIndependentSphOn, r.hp.fac_mu,
                                                                                   static_cast<shq_hydro_query *>(d_out));
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}
