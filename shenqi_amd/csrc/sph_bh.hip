/* sph_bh.hip — black-hole accretion and feedback on the walk of sph_walk.hpp: one kernel body per walk, each in three routes (write
 * on the neighbours' side, count the writes, emit them as records), and the marked-particle lists and row gathers their callers read
 * the changed particles back with; at the end the owner-side resolve and apply kernels of the record route, for a multi-rank driver. */
#include "sph_walk.hpp"
#include "device_prims.hpp"

/* ---- black-hole accretion and feedback: libgadget/blackhole.cpp:373-1003 ------------------------------
 * The two legacy-API tree walks of blackhole(): symmetric neighbour search over gas + black holes (treewalk_visit_ngbiter,
 * treewalk.c:925-975: r2 <= max(Hsml_i, Hsml_j)^2), one black hole per lane on the wave-collective walk of the SPH operators.
 *   accretion (ngbiter :471-631, postprocess :373-468): merger marks (BH_SwallowID, the reference's compare-and-swap rule),
 *     stochastic gas swallowing marks (SPH_SwallowID = the largest ID + 1 that drew the particle), the kernel-weighted entropy, gas
 *     velocity and feedback weight around the hole, Bondi-Hoyle rate capped at the Eddington factor, drag, kinetic-feedback state;
 *   feedback (ngbiter :728-876, postprocess :929-965): the marked mergers and gas particles are swallowed (mass, momentum, progenitor
 *     count), thermal energy goes into the unswallowed gas inside the kernel (compare-and-swap on the entropy, temperature cap) or
 *     the accumulated kinetic energy kicks it in a random direction, the hole takes the smallest neighbour time bin.
 * Black-hole slot fields travel as one record per black hole of the particle set, in ascending particle order. */
__device__ __forceinline__ bool bh_timebin_active(int bin, long long cur) /* is_timebin_active, timestep.cpp:132-139 */
{
    if(bin <= 0 || cur <= 0)
        return true;
    return cur % (1ll << bin) == 0;
}

/* ---- the three routes of a walk ---------------------------------------------------------------------------------------------------
 * Both walks write on the neighbours' side (marks, flags, entropy, kicks), and a neighbour may be an imported copy of another rank's
 * particle.  Each walk is one kernel body whose neighbour-side writes are chosen at compile time:
 *   BH_WRITE  they are performed inside the kernel (atomics, compare-and-swap loops): the one-shot calls;
 *   BH_COUNT  they are counted, no hole-side sums, no w.out row: the first pass of a multi-rank driver (shenqi_amd/dist.py:DistBlackHole);
 *   BH_EMIT   they are emitted as one record per (neighbour, hole) beside the hole-side sums and the w.out row: its second pass.
 * The emitted records are rewritten to (owner, row at the owner, position of the hole in the global queue) and sorted by these three
 * (shq_route_sort).  The owner sorts what it gathered by (row, hole) and one lane per particle runs over its records in ascending hole
 * order: the reference's mark rule and energy injection as a serial loop over the global queue, the same bits on every run.  No
 * floating-point atomic and no compare-and-swap loop in the BH_COUNT and BH_EMIT instantiations. */
enum BhRoute { BH_WRITE, BH_COUNT, BH_EMIT };

struct BhEmitArgs {
    unsigned long long *cursor;
    unsigned long long capacity;
    unsigned long long *keys; /* particle << 32 | queue position */
    unsigned long long *val;  /* the marking hole's ID, or the bits of the double */
    uint32_t *kind;
};

template <int ROUTE>
__device__ __forceinline__ void bh_emit(const BhEmitArgs &e, unsigned int &mine, long long p, long long t, uint32_t kind, unsigned long long bits)
{
    static_assert(ROUTE != BH_WRITE, "the write route has no records");
    if(ROUTE == BH_COUNT) {
        mine++;
        return;
    }
    const unsigned long long k = atomicAdd(e.cursor, 1ull);
    if(k < e.capacity) {
        e.keys[k] = ((unsigned long long) (unsigned) p << 32) | (unsigned long long) t;
        e.val[k] = bits;
        e.kind[k] = kind;
    }
}

__device__ __forceinline__ void bh_emit_count(const BhEmitArgs &e, unsigned int mine, int lane)
{
    for(int off = 32; off > 0; off >>= 1)
        mine += __shfl_xor(mine, off);
    if(lane == 0 && mine)
        atomicAdd(e.cursor, (unsigned long long) mine);
}

/* the accretion walk.  Its records: kind 0 on a hole (a merger candidate: close enough and the reposition / check_grav_bound flag),
 * kind 1 on a gas particle (the draw succeeded); both carry the marking hole's ID */
#define BH_ACC_NOUT 8
template <int KT, int ROUTE>
__global__ __launch_bounds__(256) void bh_accretion_kernel(const SphDev a, const int32_t *queue, long long nq, const BhWalkArgs w, const shq_kick_factors kf,
                                                           const BhEmitArgs e, int32_t *__restrict__ nlist, long long ntasks)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(32))) char lds[4 * NW_LDS_PER_WAVE(true)];
    const int lane = threadIdx.x & 63;
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = wave * 64 + lane;
    const bool valid = t < nq;
    double px = 0, py = 0, pz = 0, h = 1, imass = 0, ibhmass = 0, idens = 0, imtrack = 0;
    double iv[3] = {0, 0, 0}, ia[3] = {0, 0, 0};
    unsigned long long myid = 0;
    if(valid) {
        const long long pi = queue[t];
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z;
        imass = p.w;
        h = a.hsml[pi];
        myid = w.ids[pi];
        const long long b = shq_bh_ordinal(w.bhp, w.nbh, (int32_t) pi);
        const BhRec &B = w.bh[b];
        ibhmass = B.Mass; idens = B.Density; imtrack = B.Mtrack;
        for(int d = 0; d < 3; d++) {
            iv[d] = w.vel[3 * pi + d];
            ia[d] = w.treeacc[3 * pi + d] + w.gravpm[3 * pi + d] + B.DFAccel[d]; /* blackhole_accretion_copy, :661-662 */
        }
    }
    const Kern<KT> kernel(h);
    const double HH = kernel.H * kernel.H, Hinv = 1.0 / kernel.H;
    const double h2 = h * h;
    int encounter = 0;
    unsigned int mine = 0;
    double fws = 0, sment = 0, gv0 = 0, gv1 = 0, gv2 = 0, mgas = 0;
    const double rmerge = 2 * w.P.ForceSoftening / 2.8;
    auto pair = [&](const int s) {
        const long long p = w.leaf_pidx[s];
        const double4 q = a.posm_leaf[s];
        const int type = w.pflags[p] >> 4;
        if(q.w < 0)
            return;
        if(w.P.WindsDecoupleSph && type == 0 && w.delay[p] > 0) /* winds_is_particle_decoupled */
            return;
        if(w.ids[p] == myid)
            return;
        const double d0 = wrapd(px - q.x, a.Box, a.invBox), d1 = wrapd(py - q.y, a.Box, a.invBox), d2 = wrapd(pz - q.z, a.Box, a.invBox);
        const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
        const double r = sqrt(r2);
        if(type == 5 && r < rmerge) {
            encounter = 1;
            const long long ob = shq_bh_ordinal(w.bhp, w.nbh, (int32_t) p);
            int flag = 0;
            if(w.P.RepositionEnabled == 1 || w.P.MergeGravBound == 0)
                flag = 1;
            if(w.P.MergeGravBound == 1 && w.P.RepositionEnabled == 0 && ob >= 0) {
                /* check_grav_bound, :160-180, with DM_VelPred of the other hole */
                const double dx[3] = {d0, d1, d2};
                double KE = 0, PE = 0;
                const int bg = w.bin_grav[p];
                for(int d = 0; d < 3; d++) {
                    const double vp = w.vel[3 * p + d] + kf.gravkicks[bg] * w.treeacc[3 * p + d] + w.gravpm[3 * p + d] * kf.FgravkickB;
                    const double dv = iv[d] - vp;
                    const double da = ia[d] - w.treeacc[3 * p + d] - w.gravpm[3 * p + d] - w.bh[ob].DFAccel[d];
                    KE += 0.5 * (dv * dv);
                    PE += da * dx[d];
                }
                KE /= (w.P.atime * w.P.atime);
                PE /= w.P.atime;
                flag = (PE + KE <= 0);
            }
            if(flag == 1 && ob >= 0) {
                if constexpr(ROUTE == BH_WRITE) {
                    const unsigned long long oid = w.ids[p];
                    const bool oactive = bh_timebin_active(w.bin_hydro[p], w.Ti_Current);
                    unsigned long long *swal = w.bh_swallow + ob;
                    unsigned long long readid = atomicAdd(swal, 0ull);
                    for(;;) {
                        unsigned long long newid;
                        if(readid != 0 && readid < myid)
                            newid = myid + 1;
                        else if(readid == 0 && (oid < myid || !oactive))
                            newid = myid + 1;
                        else
                            break;
                        const unsigned long long seen = atomicCAS(swal, readid, newid);
                        if(seen == readid)
                            break;
                        readid = seen;
                    }
                } else
                    bh_emit<ROUTE>(e, mine, p, t, 0u, myid);
            }
        }
        if(type == 0 && r2 < HH) {
            const double u = r * Hinv;
            const double wk = kernel.wk(u);
            const double mass_j = q.w;
            if constexpr(ROUTE != BH_COUNT) {
                sment += (mass_j * wk * w.entropy[p]);
                const double4 vp = a.velp[p]; /* SPH_VelPred */
                gv0 += (mass_j * wk * vp.x);
                gv1 += (mass_j * wk * vp.y);
                gv2 += (mass_j * wk * vp.z);
            }
            double pacc = 0;
            double BHPartMass = imass;
            if(w.P.SeedBHDynMass > 0 && imtrack < w.P.SeedBHDynMass)
                BHPartMass = imtrack;
            if((ibhmass - BHPartMass) > 0 && idens > 0)
                pacc = (ibhmass - BHPartMass) * wk / idens;
            const double rn = w.rnd[w.ids[p] % w.rndsize];
            if constexpr(ROUTE == BH_WRITE) {
                if(rn < pacc)
                    atomicMax(w.sph_swallow + p, myid + 1); /* "prefer to be swallowed by a bigger ID" */
                if(w.touched) /* every gas neighbour inside the kernel: a superset of the marked ones (could be narrowed to rn < pacc) */
                    w.touched[p] = 1;
            } else if(rn < pacc)
                bh_emit<ROUTE>(e, mine, p, t, 1u, myid);
            if constexpr(ROUTE != BH_COUNT) {
                fws += (mass_j * wk);
                if(w.P.BlackHoleKineticOn == 1)
                    mgas += mass_j;
            }
        }
    };
    auto accept = [&](const double r2, const double hj, const int) { return r2 <= h2 || r2 <= hj * hj; };
    int fill = 0;
    bool ovf = false;
    (void) ngb_walk<true, false, false>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(true), myl, valid, px, py, pz, h, accept, pair,
                                        (unsigned int *) nullptr, fill, ovf);
    if constexpr(ROUTE == BH_COUNT)
        bh_emit_count(e, mine, lane);
    else if(valid) {
        double *o = w.out + BH_ACC_NOUT * t;
        o[0] = encounter; o[1] = fws; o[2] = sment; o[3] = gv0; o[4] = gv1; o[5] = gv2; o[6] = mgas; o[7] = 0;
    }
    } /* task loop */
}

/* blackhole_accretion_postprocess (:373-468), one thread per active black hole; out[t] then holds BH_Entropy and
 * BH_SurroundingGasVel normalised, and the hole's record Mdot, Mass, DragAccel (in out), KineticFdbkEnergy, KEflag */
__global__ void bh_accretion_post_kernel(long long nq, const int32_t *queue, const BhWalkArgs w, const shq_kick_factors kf, const double4 *posm, double *post)
{
#pragma clang fp contract(off)
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nq)
        return;
    const long long i = queue[t];
    const long long b = shq_bh_ordinal(w.bhp, w.nbh, (int32_t) i);
    BhRec &B = w.bh[b];
    double *o = w.out + BH_ACC_NOUT * t;
    const shq_bh_params &P = w.P;
    double mdot = 0;
    const double meddington = P.EddingtonConst * B.Mass * P.UnitTime_in_s / P.HubbleParam;
    B.FeedbackWeightSum = o[1];
    double ent = o[2], gv[3] = {o[3], o[4], o[5]};
    if(B.Density > 0) {
        ent /= B.Density;
        for(int k = 0; k < 3; k++)
            gv[k] /= B.Density;
        double bhvel = 0;
        for(int k = 0; k < 3; k++) {
            const double dv = w.vel[3 * i + k] - gv[k];
            bhvel += dv * dv;
        }
        bhvel = sqrt(bhvel);
        bhvel /= P.atime;
        const double rho = B.Density;
        const double rho_proper = rho * P.a3inv;
        double soundspeed = 0; /* blackhole_soundspeed, :147-157 */
        if(rho > 0) {
            soundspeed = sqrt(SPH_GAMMA * ent * pow(rho, SPH_GAMMA - 1));
            soundspeed *= pow(P.atime, -1.5 * (SPH_GAMMA - 1));
        }
        const double norm = pow((soundspeed * soundspeed + bhvel * bhvel), 1.5);
        if(norm > 0)
            mdot = 4. * M_PI * P.BlackHoleAccretionFactor * P.GravInternal * P.GravInternal * B.Mass * B.Mass * rho_proper / norm;
    }
    if(P.BlackHoleEddingtonFactor > 0.0 && mdot > P.BlackHoleEddingtonFactor * meddington)
        mdot = P.BlackHoleEddingtonFactor * meddington;
    B.Mdot = mdot;
    const double dtime = kf.dloga_for_bin[w.bin_hydro[i]] / P.hubble;
    B.Mass += B.Mdot * dtime;
    double drag[3] = {0, 0, 0};
    if(P.BH_DRAG > 0) {
        double fac = 0;
        if(P.BH_DRAG == 1)
            fac = B.Mdot / posm[i].w;
        if(P.BH_DRAG == 2)
            fac = P.BlackHoleEddingtonFactor * meddington / B.Mass;
        fac *= P.atime;
        for(int k = 0; k < 3; k++)
            drag[k] = -(w.vel[3 * i + k] - gv[k]) * fac;
    }
    B.KEflag = 0;
    if(P.BlackHoleKineticOn == 1) {
        const double Edd_ratio = B.Mdot / meddington;
        double lam_thresh = P.BHKE_EddingtonThrFactor;
        const double x = P.BHKE_EddingtonMFactor * pow(B.Mass / P.BHKE_EddingtonMPivot, P.BHKE_EddingtonMIndex);
        if(lam_thresh > x)
            lam_thresh = x;
        if(Edd_ratio < lam_thresh) {
            B.KEflag = 1;
            const double rho_crit_baryon = P.OmegaBaryon * 3 * (P.Hubble * P.Hubble) / (8 * M_PI * P.GravInternal);
            const double rho_sfr = P.BHKE_SfrCritOverDensity * rho_crit_baryon;
            double epsilon = (B.Density / rho_sfr) / P.BHKE_EffRhoFactor;
            if(epsilon > P.BHKE_EffCap)
                epsilon = P.BHKE_EffCap;
            B.KineticFdbkEnergy += epsilon * (B.Mdot * dtime * (P.LightOverUnitVel * P.LightOverUnitVel));
        }
        double KE_thresh = 0.5 * B.VDisp * B.VDisp * o[6];
        KE_thresh *= P.BHKE_InjEnergyThr;
        if(B.VDisp > 0 && B.KineticFdbkEnergy > KE_thresh)
            B.KEflag = 2;
    }
    double *q = post + 8 * t;
    q[0] = ent; q[1] = gv[0]; q[2] = gv[1]; q[3] = gv[2]; q[4] = drag[0]; q[5] = drag[1]; q[6] = drag[2]; q[7] = 0;
}

__global__ void bh_gather_leaf_kernel(long long nleaf, const int32_t *__restrict__ pidx, const uint8_t *__restrict__ pflags, int32_t *flag_leaf)
{
    const long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(s >= nleaf)
        return;
    const unsigned f = pflags[pidx[s]];
    const int type = f >> 4;
    flag_leaf[s] = ((f & 1u) || !(type == 0 || type == 5)) ? 1 : 0; /* IsGarbage; GASMASK + BHMASK (treewalk.c:943-949) */
}

/* the feedback walk.  Its records: kind 0 this hole swallows the hole, kind 1 it swallows the gas particle, kind 2 heat
 * (injected / mass_j), kind 3 kick (dvel).  w.bh_swallow / w.sph_swallow are the resolved marks. */
#define BH_FB_NOUT 8
template <int KT, int ROUTE>
__global__ __launch_bounds__(256) void bh_feedback_kernel(const SphDev a, const int32_t *queue, long long nq, const BhWalkArgs w, const shq_kick_factors kf,
                                                          const BhEmitArgs e, int32_t *__restrict__ nlist, long long ntasks)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(32))) char lds[4 * NW_LDS_PER_WAVE(true)];
    const int lane = threadIdx.x & 63;
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = wave * 64 + lane;
    const bool valid = t < nq;
    double px = 0, py = 0, pz = 0, h = 1, idens = 0, imtrack = 0, fws = 0, fbenergy = 0, kefb = 0;
    int channel = 0;
    unsigned long long myid = 0;
    if(valid) {
        const long long pi = queue[t];
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z;
        h = a.hsml[pi];
        myid = w.ids[pi];
        const long long b = shq_bh_ordinal(w.bhp, w.nbh, (int32_t) pi);
        const BhRec &B = w.bh[b];
        idens = B.Density; imtrack = B.Mtrack;
        fws = B.FeedbackWeightSum;
        /* blackhole_feedback_copy, :886-909 */
        const double dtime = kf.dloga_for_bin[w.bin_hydro[pi]] / w.P.hubble;
        fbenergy = w.P.BlackHoleFeedbackFactor * 0.1 * B.Mdot * dtime * (w.P.LightOverUnitVel * w.P.LightOverUnitVel);
        if(w.P.BlackHoleKineticOn == 1 && B.KEflag > 0) {
            channel = 1;
            if(B.KEflag == 2)
                kefb = B.KineticFdbkEnergy;
        }
    }
    const Kern<KT> kernel(h);
    const double HH = kernel.H * kernel.H, Hinv = 1.0 / kernel.H;
    const double h2 = h * h;
    int mintimebin = SHQ_TIMEBINS, countprogs = 0;
    unsigned int mine = 0;
    double accmass = 0, accbh = 0, mom0 = 0, mom1 = 0, mom2 = 0;
    auto pair = [&](const int s) {
        const long long p = w.leaf_pidx[s];
        const double4 q = a.posm_leaf[s];
        const int type = w.pflags[p] >> 4;
        if(w.ids[p] == myid)
            return;
        if(w.P.WindsDecoupleSph && type == 0 && w.delay[p] > 0)
            return;
        if(type == 5) {
            const long long ob = shq_bh_ordinal(w.bhp, w.nbh, (int32_t) p);
            if(ob < 0 || w.bh_swallow[ob] == 0)
                return;
            if(w.bh_swallow[ob] != myid + 1)
                return;
            if constexpr(ROUTE == BH_WRITE) {
                w.bh_swallowid_out[ob] = w.bh_swallow[ob] - 1;
                atomicOr(reinterpret_cast<unsigned int *>(w.pflags + (p & ~3ll)), 2u << (8 * (p & 3))); /* Swallowed = 1 */
            } else
                bh_emit<ROUTE>(e, mine, p, t, 0u, 0ull);
            if constexpr(ROUTE != BH_COUNT) {
                const BhRec &O = w.bh[ob];
                countprogs += O.CountProgs;
                accbh += O.Mass;
                double othermass = q.w;
                if(w.P.SeedBHDynMass > 0 && imtrack > 0)
                    if(O.Mtrack < w.P.SeedBHDynMass)
                        othermass = O.Mtrack;
                accmass += othermass;
                const int bg = w.bin_grav[p];
                const double v0 = w.vel[3 * p] + kf.gravkicks[bg] * w.treeacc[3 * p] + w.gravpm[3 * p] * kf.FgravkickB;
                const double v1 = w.vel[3 * p + 1] + kf.gravkicks[bg] * w.treeacc[3 * p + 1] + w.gravpm[3 * p + 1] * kf.FgravkickB;
                const double v2 = w.vel[3 * p + 2] + kf.gravkicks[bg] * w.treeacc[3 * p + 2] + w.gravpm[3 * p + 2] * kf.FgravkickB;
                mom0 += (othermass * v0);
                mom1 += (othermass * v1);
                mom2 += (othermass * v2);
            }
            return;
        }
        if(type != 0)
            return;
        const double d0 = wrapd(px - q.x, a.Box, a.invBox), d1 = wrapd(py - q.y, a.Box, a.invBox), d2 = wrapd(pz - q.z, a.Box, a.invBox);
        const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
        const unsigned long long mark = w.sph_swallow[p];
        if(mark == 0 && r2 < HH) {
            const int bh = w.bin_hydro[p];
            if(mintimebin > bh)
                mintimebin = bh;
            const double u = sqrt(r2) * Hinv;
            const double mass_j = q.w;
            const double wk = kernel.wk(u);
            if(fws > 0 && fbenergy > 0 && channel == 0 && mass_j > 0) {
                const double injected = fbenergy * mass_j * wk / fws;
                if constexpr(ROUTE == BH_WRITE) {
                    if(w.eeqos && w.eeqos[p])
                        w.heated[p] = 1;
                    if(w.touched)
                        w.touched[p] = 1;
                    const double enttou = pow(w.density[p] * w.P.a3inv, SPH_GAMMA - 1) / (SPH_GAMMA - 1);
                    unsigned long long *eptr = reinterpret_cast<unsigned long long *>(w.entropy + p);
                    unsigned long long oldb = atomicAdd(eptr, 0ull);
                    for(;;) {
                        /* add_injected_BH_energy, :700-710 */
                        double unew = __longlong_as_double((long long) oldb) * enttou;
                        unew += injected / mass_j;
                        if(unew > w.P.MaxThermalU)
                            unew = w.P.MaxThermalU;
                        const double entnew = unew / enttou;
                        const unsigned long long seen = atomicCAS(eptr, oldb, (unsigned long long) __double_as_longlong(entnew));
                        if(seen == oldb)
                            break;
                        oldb = seen;
                    }
                } else
                    bh_emit<ROUTE>(e, mine, p, t, 2u, (unsigned long long) __double_as_longlong(injected / mass_j));
            }
            if(kefb > 0 && channel == 1 && idens > 0) {
                const double dvel = sqrt(2 * kefb * wk / idens);
                if constexpr(ROUTE == BH_WRITE) {
                    /* get_random_dir, :712-723 */
                    const double theta = acos(2 * w.rnd[(w.ids[p] + 3) % w.rndsize] - 1);
                    const double phi = 2 * M_PI * w.rnd[(w.ids[p] + 4) % w.rndsize];
                    const double dir[3] = {sin(theta) * cos(phi), sin(theta) * sin(phi), cos(theta)};
                    for(int j = 0; j < 3; j++)
                        atomicAdd(w.velw + 3 * p + j, dvel * dir[j]);
                    if(w.touched)
                        w.touched[p] = 1;
                } else
                    bh_emit<ROUTE>(e, mine, p, t, 3u, (unsigned long long) __double_as_longlong(dvel));
            }
        }
        if(mark == myid + 1) {
            if constexpr(ROUTE == BH_WRITE) {
                if(w.touched)
                    w.touched[p] = 1;
                atomicOr(reinterpret_cast<unsigned int *>(w.pflags + (p & ~3ll)), 1u << (8 * (p & 3))); /* slots_mark_garbage */
            } else
                bh_emit<ROUTE>(e, mine, p, t, 1u, 0ull);
            if constexpr(ROUTE != BH_COUNT) {
                accmass += q.w;
                const double4 vp = a.velp[p];
                mom0 += (q.w * vp.x);
                mom1 += (q.w * vp.y);
                mom2 += (q.w * vp.z);
            }
        }
    };
    auto accept = [&](const double r2, const double hj, const int) { return r2 <= h2 || r2 <= hj * hj; };
    int fill = 0;
    bool ovf = false;
    (void) ngb_walk<true, false, false>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(true), myl, valid, px, py, pz, h, accept, pair,
                                        (unsigned int *) nullptr, fill, ovf);
    if constexpr(ROUTE == BH_COUNT)
        bh_emit_count(e, mine, lane);
    else if(valid) {
        double *o = w.out + BH_FB_NOUT * t;
        o[0] = accmass; o[1] = accbh; o[2] = mom0; o[3] = mom1; o[4] = mom2; o[5] = countprogs; o[6] = mintimebin; o[7] = 0;
    }
    } /* task loop */
}

/* blackhole_feedback_postprocess (:929-965), one thread per hole of the feedback queue; out[t] = accreted mass, accreted black-hole
 * mass, momentum[3], progenitors, minTimeBin from the walk */
__global__ void bh_feedback_post_kernel(long long nq, const int32_t *queue, const BhWalkArgs w, double4 *posm)
{
#pragma clang fp contract(off)
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nq)
        return;
    const long long n = queue[t];
    const long long b = shq_bh_ordinal(w.bhp, w.nbh, (int32_t) n);
    BhRec &B = w.bh[b];
    const double *o = w.out + BH_FB_NOUT * t;
    B.CountProgs += (int32_t) o[5];
    if(o[1] > 0)
        B.Mass += o[1];
    if(o[0] > 0) {
        const double accmass = o[0];
        const float pm = (float) posm[n].w;
        for(int k = 0; k < 3; k++)
            w.velw[3 * n + k] = (w.velw[3 * n + k] * pm + o[2 + k]) / (pm + accmass);
        const double SeedBHDynMass = w.P.SeedBHDynMass;
        if(SeedBHDynMass > 0 && B.Mtrack + accmass < SeedBHDynMass)
            B.Mtrack += accmass;
        else if(B.Mtrack < SeedBHDynMass) {
            posm[n].w = (double) (float) (B.Mtrack + accmass);
            B.Mtrack = SeedBHDynMass;
        } else
            posm[n].w = (double) (float) (pm + accmass);
    }
    if(B.KEflag == 2)
        B.KineticFdbkEnergy = 0;
}

int sph_gather_gas_flags(shq_context *ctx)
{
    const long long nl = ctx->ntreeparts + SHQ_NMAXCHILD;
    bh_gather_leaf_kernel<<<dim3(nblk(nl)), dim3(256), 0, ctx->stream>>>(nl, ctx->leaf_pidx.ptr, ctx->pflags.ptr, ctx->flag_leaf.ptr);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* what a walk needs before its first launch of a call: SPH_VelPred of every gas particle, Hsml in leaf order, the leaf flags, the lists */
static int bh_walk_prep(shq_context *ctx, const shq_kick_factors *kf, const BhWalkArgs *w)
{
    const int kt = w->P.DensityKernelType;
    SHQ_CHECK(kt == 1 || kt == 2 || kt == 4, SHQ_ERR_INVALID, "unknown DensityKernelType %d", kt);
    SHQ_TRY(shq_sph_prepare(ctx, kf, nullptr, nullptr));
    SHQ_TRY(sph_gather_gas_flags(ctx));
    return sph_reserve_nlist2(ctx);
}

/* one walk (feedback, else accretion) in one route and, where the route has hole-side sums, its postprocess; timed as the count pass or
 * as the walk */
template <int ROUTE>
static int bh_walk_launch(shq_context *ctx, const shq_kick_factors *kf, const BhWalkArgs *w, bool feedback, const int32_t *d_queue, int64_t nq, const BhEmitArgs &e,
                          double *d_post)
{
    hipStream_t st = ctx->stream;
    SphDev a = make_dev(ctx, w->P.BoxSize);
    const long long ntasks = (nq + 255) / 256;
    const unsigned grid = (unsigned) (ntasks < NL_REDO_BLOCKS ? ntasks : NL_REDO_BLOCKS);
    const int timer = ROUTE == BH_COUNT ? SHQ_T_BH_COUNT : SHQ_T_BH;
    void (*walk)(SphDev, const int32_t *, long long, BhWalkArgs, shq_kick_factors, BhEmitArgs, int32_t *, long long);
    switch(w->P.DensityKernelType) {
    case 1: walk = feedback ? bh_feedback_kernel<1, ROUTE> : bh_accretion_kernel<1, ROUTE>; break;
    case 2: walk = feedback ? bh_feedback_kernel<2, ROUTE> : bh_accretion_kernel<2, ROUTE>; break;
    default: walk = feedback ? bh_feedback_kernel<4, ROUTE> : bh_accretion_kernel<4, ROUTE>; break;
    }
    SHQ_HIP(hipEventRecord(ctx->ev_begin[timer], st));
    walk<<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, *kf, e, ctx->s_nlist2.ptr, ntasks);
    SHQ_HIP(hipGetLastError());
    if(ROUTE != BH_COUNT) {
        if(feedback)
            bh_feedback_post_kernel<<<dim3(nblk(nq)), dim3(256), 0, st>>>(nq, d_queue, *w, ctx->posm.ptr);
        else
            bh_accretion_post_kernel<<<dim3(nblk(nq)), dim3(256), 0, st>>>(nq, d_queue, *w, *kf, ctx->posm.ptr, d_post);
        SHQ_HIP(hipGetLastError());
    }
    SHQ_HIP(hipEventRecord(ctx->ev_end[timer], st));
    return SHQ_OK;
}

int shq_bh_accretion_device(shq_context *ctx, const shq_kick_factors *kf, const BhWalkArgs *w, const int32_t *d_queue, int64_t nq, double *d_post)
{
    if(nq == 0)
        return SHQ_OK;
    SHQ_TRY(bh_walk_prep(ctx, kf, w));
    return bh_walk_launch<BH_WRITE>(ctx, kf, w, false, d_queue, nq, BhEmitArgs{}, d_post);
}

int shq_bh_feedback_device(shq_context *ctx, const shq_kick_factors *kf, const BhWalkArgs *w, const int32_t *d_queue, int64_t nq)
{
    if(nq == 0)
        return SHQ_OK;
    SHQ_TRY(bh_walk_prep(ctx, kf, w));
    return bh_walk_launch<BH_WRITE>(ctx, kf, w, true, d_queue, nq, BhEmitArgs{}, nullptr);
}

namespace {
struct Marked {
    const uint8_t *mark;
    __device__ bool operator()(const int32_t &i) const { return mark[i] != 0; }
};
__global__ void rows_gather_kernel(long long m, const int32_t *__restrict__ list, const double *__restrict__ vel, const double *__restrict__ entropy,
                                   const double *__restrict__ delay, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                   const uint8_t *__restrict__ extra, double *rows)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= m)
        return;
    const long long p = list[t];
    double *r = rows + 8 * t;
    r[0] = vel[3 * p];
    r[1] = vel[3 * p + 1];
    r[2] = vel[3 * p + 2];
    r[3] = entropy ? entropy[p] : 0.0;
    r[4] = delay ? delay[p] : 0.0;
    r[5] = posm[p].w;
    r[6] = (double) pflags[p];
    r[7] = extra ? (double) extra[p] : 0.0;
}
} // namespace

int shq_marked_list(shq_context *ctx, const uint8_t *d_mark, int64_t n, int32_t *d_list, int64_t *m)
{
    *m = 0;
    if(n <= 0)
        return SHQ_OK;
    SHQ_TRY(ctx->s_counters.reserve(8));
    return prim_select_if(ctx, rocprim::counting_iterator<int32_t>(0), d_list, (size_t) n, Marked{d_mark},
                          reinterpret_cast<unsigned long long *>(ctx->s_counters.ptr), m);
}

namespace {
__global__ void u64_gather_kernel(long long m, const int32_t *__restrict__ list, const unsigned long long *__restrict__ src, unsigned long long *out)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t < m)
        out[t] = src[list[t]];
}
} // namespace

int shq_u64_gather(shq_context *ctx, const int32_t *d_list, int64_t m, const unsigned long long *d_src, unsigned long long *d_out)
{
    if(m <= 0)
        return SHQ_OK;
    u64_gather_kernel<<<dim3(nblk(m)), dim3(256), 0, ctx->stream>>>(m, d_list, d_src, d_out);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

int shq_rows_gather(shq_context *ctx, const int32_t *d_list, int64_t m, const uint8_t *d_extra, double *d_rows)
{
    if(m <= 0)
        return SHQ_OK;
    rows_gather_kernel<<<dim3(nblk(m)), dim3(256), 0, ctx->stream>>>(m, d_list, ctx->vel.ptr, ctx->g_entropy.ptr, ctx->g_delaytime.ptr, ctx->posm.ptr,
                                                                      ctx->pflags.ptr, d_extra, d_rows);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}


/* ---- the record routes of the two walks, for a multi-rank driver ---------------------------------------------------------------- */
static int bh_cursor_read(shq_context *ctx, unsigned long long *h)
{
    SHQ_HIP(hipMemcpyAsync(h, ctx->wind_cnt.ptr, sizeof(*h), hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    return SHQ_OK;
}

int shq_bh_records_count_device(shq_context *ctx, const shq_kick_factors *kf, const BhWalkArgs *w, bool effects, const int32_t *d_queue, int64_t nq, int64_t *nrec)
{
    *nrec = 0;
    if(nq == 0)
        return SHQ_OK;
    SHQ_TRY(bh_walk_prep(ctx, kf, w));
    SHQ_TRY(ctx->wind_cnt.reserve(4));
    SHQ_HIP(hipMemsetAsync(ctx->wind_cnt.ptr, 0, sizeof(unsigned long long), ctx->stream));
    BhEmitArgs e;
    memset(&e, 0, sizeof(e));
    e.cursor = ctx->wind_cnt.ptr;
    SHQ_TRY(bh_walk_launch<BH_COUNT>(ctx, kf, w, effects, d_queue, nq, e, nullptr));
    unsigned long long h = 0;
    SHQ_TRY(bh_cursor_read(ctx, &h));
    *nrec = (int64_t) h;
    return SHQ_OK;
}

namespace {
__global__ void bh_record_write_kernel(long long n, const uint32_t *__restrict__ owner_sorted, const uint32_t *__restrict__ ord, const unsigned long long *__restrict__ routed,
                                       const uint32_t *__restrict__ kind, const unsigned long long *__restrict__ val, shq_bh_record *out)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    const size_t j = ord[k];
    shq_bh_record R;
    R.owner = (int32_t) owner_sorted[k];
    R.part_index = (int32_t) (routed[j] >> 32);
    R.hole = (uint32_t) (routed[j] & 0xffffffffull);
    R.kind = (int32_t) kind[j];
    R.bits = val[j];
    out[k] = R;
}
} // namespace

/* the emit pass for the nrec records the count pass found, the hole-side postprocess (d_post: accretion's, NULL for the feedback's),
 * and the routed, sorted list in ctx->metal_trip with the per-owner counts in d_counts[nranks] */
int shq_bh_records_emit_device(shq_context *ctx, const shq_kick_factors *kf, const BhWalkArgs *w, bool effects, const int32_t *d_queue, int64_t nq, int64_t nrec,
                               int64_t nlocal, const int32_t *d_ghost_owner, const int32_t *d_ghost_index, int nranks, int rank, int64_t queue_offset,
                               const int32_t *d_qpos, unsigned long long *d_counts, double *d_post)
{
    hipStream_t st = ctx->stream;
    SHQ_HIP(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * (size_t) nranks, st));
    if(nq == 0)
        return SHQ_OK;
    SHQ_CHECK(nrec < (1ll << 32), SHQ_ERR_INVALID, "%lld black-hole records, the sort orders are 32 bits", (long long) nrec);
    const size_t m = (size_t) std::max<int64_t>(nrec, 1);
    SHQ_TRY(ctx->metal_keys[0].reserve(m));
    SHQ_TRY(ctx->metal_keys[1].reserve(m));
    SHQ_TRY(ctx->metal_val[0].reserve(m));
    SHQ_TRY(ctx->bhd_kind.reserve(m));
    for(auto &b : ctx->metal_u32)
        SHQ_TRY(b.reserve(m));
    SHQ_TRY(ctx->metal_trip.reserve(m * sizeof(shq_bh_record)));
    SHQ_HIP(hipMemsetAsync(ctx->wind_cnt.ptr, 0, sizeof(unsigned long long), st));
    BhEmitArgs e;
    e.cursor = ctx->wind_cnt.ptr;
    e.capacity = (unsigned long long) nrec;
    e.keys = ctx->metal_keys[0].ptr;
    e.val = reinterpret_cast<unsigned long long *>(ctx->metal_val[0].ptr);
    e.kind = ctx->bhd_kind.ptr;
    SHQ_TRY(bh_walk_launch<BH_EMIT>(ctx, kf, w, effects, d_queue, nq, e, d_post));
    unsigned long long h = 0;
    SHQ_TRY(bh_cursor_read(ctx, &h));
    SHQ_CHECK(h == (unsigned long long) nrec, SHQ_ERR_STATE, "black-hole records: the two walks disagree on their number (%lld, %llu)", (long long) nrec, h);
    SHQ_HIP(hipEventRecord(ctx->ev_begin[SHQ_T_BH_ROUTE], st));
    if(nrec > 0) {
        SHQ_TRY(shq_route_sort(ctx, nrec, nlocal, d_ghost_owner, d_ghost_index, nranks, rank, queue_offset, d_qpos, d_counts));
        bh_record_write_kernel<<<dim3(nblk(nrec)), dim3(256), 0, st>>>(nrec, ctx->metal_u32[0].ptr, ctx->metal_u32[3].ptr, ctx->metal_keys[1].ptr, ctx->bhd_kind.ptr,
                                                                       reinterpret_cast<unsigned long long *>(ctx->metal_val[0].ptr),
                                                                       reinterpret_cast<shq_bh_record *>(ctx->metal_trip.ptr));
        SHQ_HIP(hipGetLastError());
    }
    SHQ_HIP(hipEventRecord(ctx->ev_end[SHQ_T_BH_ROUTE], st));
    return SHQ_OK;
}

namespace {
__global__ void bh_record_keys_kernel(long long n, const shq_bh_record *__restrict__ rec, unsigned long long *keys)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k < n)
        keys[k] = ((unsigned long long) (uint32_t) rec[k].part_index << 32) | (unsigned long long) rec[k].hole;
}

/* one lane per run of equal particles in the (row, hole)-sorted list.  A gas particle keeps the largest ID + 1 that drew it; on a hole
 * the reference's compare-and-swap rule (blackhole.cpp:570-590) runs over its candidates in ascending hole order. */
__global__ void bh_resolve_kernel(long long n, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ ord, const shq_bh_record *__restrict__ rec,
                                  const unsigned long long *__restrict__ ids, const uint8_t *__restrict__ bin_hydro, long long Ti_Current, int32_t *out_part,
                                  unsigned long long *out_mark)
{
    const long long k0 = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k0 >= n)
        return;
    const unsigned p = (unsigned) (keys[k0] >> 32);
    if(k0 > 0 && (unsigned) (keys[k0 - 1] >> 32) == p) {
        out_part[k0] = -1;
        return;
    }
    const unsigned long long oid = ids[p];
    const bool oactive = bh_timebin_active(bin_hydro[p], Ti_Current);
    unsigned long long mark = 0;
    for(long long k = k0; k < n && (unsigned) (keys[k] >> 32) == p; k++) {
        const shq_bh_record &R = rec[ord[k]];
        const unsigned long long id = R.bits;
        if(R.kind == 1) {
            if(mark < id + 1)
                mark = id + 1;
        } else if(mark != 0 && mark < id)
            mark = id + 1;
        else if(mark == 0 && (oid < id || !oactive))
            mark = id + 1;
    }
    out_part[k0] = (int32_t) p;
    out_mark[k0] = mark;
}

/* one lane per particle, its records in ascending hole order: the neighbour side of blackhole_feedback_ngbiter (:760-870) */
__global__ void bh_apply_kernel(long long n, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ ord, const shq_bh_record *__restrict__ rec,
                                const BhWalkArgs w)
{
#pragma clang fp contract(off)
    const long long k0 = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k0 >= n)
        return;
    const unsigned p = (unsigned) (keys[k0] >> 32);
    if(k0 > 0 && (unsigned) (keys[k0 - 1] >> 32) == p)
        return;
    for(long long k = k0; k < n && (unsigned) (keys[k] >> 32) == p; k++) {
        const shq_bh_record &R = rec[ord[k]];
        const double value = __longlong_as_double((long long) R.bits);
        if(R.kind == 0)
            w.pflags[p] |= 2u; /* Swallowed */
        else if(R.kind == 1)
            w.pflags[p] |= 1u; /* slots_mark_garbage */
        else if(R.kind == 2) {
            if(w.eeqos && w.eeqos[p])
                w.heated[p] = 1;
            /* add_injected_BH_energy, :700-710 */
            const double enttou = pow(w.density[p] * w.P.a3inv, SPH_GAMMA - 1) / (SPH_GAMMA - 1);
            double unew = w.entropy[p] * enttou;
            unew += value;
            if(unew > w.P.MaxThermalU)
                unew = w.P.MaxThermalU;
            w.entropy[p] = unew / enttou;
        } else {
            /* get_random_dir, :712-723 */
            const double theta = acos(2 * w.rnd[(w.ids[p] + 3) % w.rndsize] - 1);
            const double phi = 2 * M_PI * w.rnd[(w.ids[p] + 4) % w.rndsize];
            const double dir[3] = {sin(theta) * cos(phi), sin(theta) * sin(phi), cos(theta)};
            for(int j = 0; j < 3; j++)
                w.velw[3 * p + j] += value * dir[j];
        }
    }
}
} // namespace

/* d_rec (n records, any order) sorted by (row, hole): the sorted keys in metal_keys[1], the records' places in metal_u32[0] */
static int bh_records_sort(shq_context *ctx, const shq_bh_record *d_rec, int64_t n)
{
    SHQ_CHECK(n < (1ll << 32), SHQ_ERR_INVALID, "%lld black-hole records, the sort orders are 32 bits", (long long) n);
    SHQ_TRY(ctx->metal_keys[0].reserve((size_t) n));
    SHQ_TRY(ctx->metal_keys[1].reserve((size_t) n));
    SHQ_TRY(ctx->metal_u32[0].reserve((size_t) n));
    bh_record_keys_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(n, d_rec, ctx->metal_keys[0].ptr);
    SHQ_HIP(hipGetLastError());
    return prim_sort_pairs(ctx, ctx->metal_keys[0].ptr, ctx->metal_keys[1].ptr, rocprim::counting_iterator<uint32_t>(0), ctx->metal_u32[0].ptr, (size_t) n, 0, 64);
}

int shq_bh_resolve_device(shq_context *ctx, const shq_bh_record *d_rec, int64_t n, const unsigned long long *d_ids, const uint8_t *d_bin_hydro, int64_t Ti_Current,
                          int32_t *d_out_part, unsigned long long *d_out_mark)
{
    if(n == 0)
        return SHQ_OK;
    SHQ_HIP(hipEventRecord(ctx->ev_begin[SHQ_T_BH], ctx->stream));
    SHQ_TRY(bh_records_sort(ctx, d_rec, n));
    bh_resolve_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(n, ctx->metal_keys[1].ptr, ctx->metal_u32[0].ptr, d_rec, d_ids, d_bin_hydro, Ti_Current, d_out_part,
                                                                    d_out_mark);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipEventRecord(ctx->ev_end[SHQ_T_BH], ctx->stream));
    return SHQ_OK;
}

int shq_bh_apply_device(shq_context *ctx, const BhWalkArgs *w, const shq_bh_record *d_rec, int64_t n)
{
    if(n == 0)
        return SHQ_OK;
    SHQ_HIP(hipEventRecord(ctx->ev_begin[SHQ_T_BH], ctx->stream));
    SHQ_TRY(bh_records_sort(ctx, d_rec, n));
    bh_apply_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(n, ctx->metal_keys[1].ptr, ctx->metal_u32[0].ptr, d_rec, *w);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipEventRecord(ctx->ev_end[SHQ_T_BH], ctx->stream));
    return SHQ_OK;
}
