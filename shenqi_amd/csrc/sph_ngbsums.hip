/* sph_ngbsums.hip — neighbour sums around stars, black holes and star-forming gas on the walk of sph_walk.hpp: stellar density,
 * black-hole velocity dispersion, wind velocity dispersion, black-hole dynamical friction, and |grad rho| of the density pass. */
#include "sph_walk.hpp"

/* ---- stellar density: stellar_density2.cpp ------------------------------------------------------
 * The SPH volume weights around star particles for the metal return: a density-like walk over the gas tree that evaluates
 * NHSML = 10 trial radii per star in one pass (stellareffhsml :38-54, ngbiter :219-254), then narrows the Hsml bounds
 * (postprocess :113-154, ngb_narrow_down treewalk.c:1349-1406) until every star has DesNumNgb +- MaxNgbDeviation neighbours.
 * Same walk machinery as the density (fused variant: stars are few); the walk uses the largest trial radius throughout — the
 * reference shrinks its search radius on the way, which only skips candidates its ngbiter would reject anyway — and each
 * lane works through its neighbours in depth-first order with the reference's per-neighbour logic, including the running
 * `maxcmpte` cut. */
#define ST_NHSML 10

__device__ __forceinline__ double st_effhsml(int i, double left, double right, double Hsml, double Box)
{
    if(right > 0.99 * Box)
        right = Hsml * ((1. + ST_NHSML) / ST_NHSML);
    if(left == 0)
        left = 0.1 * Hsml;
    const double rvol = pow(right, 3), lvol = pow(left, 3);
    return pow((1. * i + 1) / (1. * ST_NHSML + 1) * (rvol - lvol) + lvol, 1. / 3);
}

struct StellarArgs {
    double Box, DesNumNgb, MaxDev;
    int SPHWeighting;
    const double *rho_leaf;   /* gas density by leaf slot */
    double *starvol;          /* by particle index */
    int32_t *todo;
    unsigned long long *hmax_tried; /* the largest trial radius any walk ran with or any star ends with, as the bits of a non-negative double */
};

template <int KT>
__global__ __launch_bounds__(256) void sph_stellar_kernel(const SphDev a, const int32_t *queue, long long nq, const StellarArgs sa,
                                                          unsigned long long *nint_total, int32_t *__restrict__ nlist, long long ntasks)
{
    __shared__ __attribute__((aligned(32))) char lds[4 * NW_LDS_PER_WAVE(false)];
    const int lane = threadIdx.x & 63;
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = wave * 64 + lane;
    const bool valid = t < nq;
    long long pi = 0;
    double px = 0, py = 0, pz = 0, h = 1, L = 0, R = sa.Box;
    if(valid) {
        pi = queue[t];
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z;
        h = a.hsml[pi];
        L = a.left[pi];
        R = a.right[pi];
    }
    double he[ST_NHSML], he2[ST_NHSML], hinv[ST_NHSML], wnorm[ST_NHSML], Ngb[ST_NHSML], Vol[ST_NHSML];
#pragma unroll
    for(int k = 0; k < ST_NHSML; k++) {
        he[k] = st_effhsml(k, L, R, h, sa.Box);
        he2[k] = he[k] * he[k];
        const Kern<KT> kr(he[k]);
        hinv[k] = 1.0 / he[k];
        wnorm[k] = kr.Wknorm;
        Ngb[k] = 0;
        Vol[k] = 0;
    }
    int maxcmpte = ST_NHSML;
    const Kern<KT> k0(1.0);

    /* ngbiter, stellar_density2.cpp:219-254 */
    auto pair = [&](const int s) {
        const double4 q = a.posm_leaf[s];
        const double d0 = wrapd(px - q.x, a.Box, a.invBox);
        const double d1 = wrapd(py - q.y, a.Box, a.invBox);
        const double d2 = wrapd(pz - q.z, a.Box, a.invBox);
        const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
        double lim = he2[0];
#pragma unroll
        for(int k = 1; k < ST_NHSML; k++)
            lim = (k == maxcmpte - 1) ? he2[k] : lim;
        if(maxcmpte == 1)
            lim = he2[0];
        if(!(r2 < lim))
            return;
        const double r = sqrt(r2);
        const double vj = q.w / sa.rho_leaf[s];
#pragma unroll
        for(int k = 0; k < ST_NHSML; k++) {
            if(k < maxcmpte && r2 < he2[k]) {
                const double wk = wnorm[k] * k0.wk_int(r * hinv[k] * (Kern<KT>::support / 2.));
                Ngb[k] += wk * ((4.0 / 3 * M_PI) * (he[k] * he[k] * he[k]));
                Vol[k] += sa.SPHWeighting ? vj * wk : vj;
            }
        }
        int first = ST_NHSML;
#pragma unroll
        for(int k = ST_NHSML - 1; k >= 0; k--)
            first = (Ngb[k] > sa.DesNumNgb) ? k : first;
        if(first < ST_NHSML)
            maxcmpte = first + 1;
    };
    const double hwalk2 = he2[ST_NHSML - 1];
    auto accept = [&](const double r2, const double, const int) { return r2 < hwalk2; };
    int fill = 0;
    bool ovf = false;
    unsigned int nint = ngb_walk<false, false, false>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(false), myl, valid, px, py, pz, he[ST_NHSML - 1],
                                                      accept, pair, (unsigned int *) nullptr, fill, ovf);
    if(valid) {
        /* StellarDensityOutput::postprocess (stellar_density2.cpp:113-154) with ngb_narrow_down (treewalk.c:1349-1406) */
        const int desi = (int) sa.DesNumNgb;
        int close = 0;
        double ngbdist = fabs(Ngb[0] - desi);
#pragma unroll
        for(int k = 1; k < ST_NHSML; k++) {
            const double nd = fabs(Ngb[k] - desi);
            if(k < maxcmpte && nd < ngbdist) {
                ngbdist = nd;
                close = k;
            }
        }
        bool stop = false;
#pragma unroll
        for(int k = 0; k < ST_NHSML; k++) {
            if(k < maxcmpte && !stop) {
                if(Ngb[k] < desi)
                    L = he[k];
                if(Ngb[k] > desi) {
                    R = he[k];
                    stop = true;
                }
            }
        }
        double hc = he[0], nc = Ngb[0], vc = Vol[0], rl = he[0], rl1 = he[0], nl = Ngb[0], nl1 = Ngb[0];
#pragma unroll
        for(int k = 1; k < ST_NHSML; k++) {
            if(k == close) { hc = he[k]; nc = Ngb[k]; vc = Vol[k]; }
            if(k == maxcmpte - 1) { rl = he[k]; nl = Ngb[k]; rl1 = he[k - 1]; nl1 = Ngb[k - 1]; }
        }
        double hs = hc;
        if(R > 0.99 * sa.Box) {
            double dngbdv = 0;
            if(maxcmpte > 1 && rl > rl1)
                dngbdv = (nl - nl1) / (pow(rl, 3) - pow(rl1, 3));
            double newh = 4 * hs;
            if(dngbdv > 0) {
                const double dngb = desi - nl;
                const double nv = pow(hs, 3) + dngb / dngbdv;
                if(pow(nv, 1. / 3) < newh)
                    newh = pow(nv, 1. / 3);
            }
            hs = newh;
        }
        if(hs > R)
            hs = R;
        if(L == 0) {
            double dngbdv = 0;
            if(he[1] > he[0])
                dngbdv = (Ngb[1] - Ngb[0]) / (pow(he[1], 3) - pow(he[0], 3));
            if(maxcmpte == 1 && he[0] > 0)
                dngbdv = Ngb[0] / pow(he[0], 3);
            if(dngbdv > 0) {
                const double dngb = desi - Ngb[0];
                const double nv = pow(hs, 3) + dngb / dngbdv;
                hs = pow(nv, 1. / 3);
            }
        }
        if(hs < L)
            hs = L;
        a.hsml[pi] = hs;
        a.left[pi] = L;
        a.right[pi] = R;
        a.numngb[pi] = nc;
        sa.starvol[pi] = vc;
        int redo = 0;
        if(nc < (sa.DesNumNgb - sa.MaxDev) || nc > (sa.DesNumNgb + sa.MaxDev))
            redo = ((R - L) < 1.0e-4 * L) ? 0 : 1;
        sa.todo[t] = redo ? (int32_t) pi : -1;
    }
    /* what a sharded caller sizes its halo by: the walk searched with he[ST_NHSML - 1], and hs is the next start */
    unsigned long long tried = valid ? (unsigned long long) __double_as_longlong(fmax(he[ST_NHSML - 1], a.hsml[pi])) : 0ull;
    for(int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(tried, off);
        tried = o > tried ? o : tried;
    }
    if(lane == 0 && tried > *(volatile unsigned long long *) sa.hmax_tried)
        atomicMax(sa.hmax_tried, tried);
    unsigned int sn = nint;
    for(int off = 32; off > 0; off >>= 1)
        sn += __shfl_xor(sn, off);
    if(lane == 0 && nint_total)
        atomicAdd(nint_total, (unsigned long long) sn);
    } /* task loop */
}

__global__ void gather_rho_leaf_kernel(long long nleaf, const int32_t *__restrict__ pidx, const double *__restrict__ density, double *out)
{
    const long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(s < nleaf)
        out[s] = density[pidx[s]];
}

int shq_sph_stellar_density_device(shq_context *ctx, const shq_stellar_params *p, const int32_t *d_queue, int64_t nq, double *d_starvol,
                                   shq_sph_stats *stats)
{
    const long long n = ctx->numpart;
    SHQ_CHECK(p->DensityKernelType == 1 || p->DensityKernelType == 2 || p->DensityKernelType == 4, SHQ_ERR_INVALID,
              "unknown DensityKernelType %d", p->DensityKernelType);
    SHQ_TRY(sph_reserve_redo(ctx));
    SHQ_TRY(sph_reserve_nlist2(ctx));
    const long long nl = ctx->ntreeparts + SHQ_NMAXCHILD;
    SHQ_TRY(ctx->hsml_leaf.reserve(nl));   /* reused as the density-by-slot array */
    SHQ_TRY(ctx->flag_leaf.reserve(nl));
    SHQ_TRY(ctx->velp_leaf.reserve(nl));
    hipStream_t st = ctx->stream;
    if(n > 0) {
        SHQ_HIP(hipMemsetAsync(ctx->s_left.ptr, 0, sizeof(double) * n, st));
        sph_fill(ctx, ctx->s_right.ptr, n, p->BoxSize);
    }
    SHQ_HIP(hipMemsetAsync(ctx->s_counters.ptr, 0, sizeof(long long) * 8, st));
    /* neighbour-side arrays in leaf order: density and the skip flags (garbage / no longer gas) */
    gather_rho_leaf_kernel<<<dim3(nblk(nl)), dim3(256), 0, st>>>(nl, ctx->leaf_pidx.ptr, ctx->g_density.ptr, ctx->hsml_leaf.ptr);
    sph_gather_leaf_plain(ctx, nl, ctx->s_evp_in.ptr); /* Hsml by slot is not read here: hsml_leaf holds the density */
    SHQ_HIP(hipGetLastError());
    SphDev a = make_dev(ctx, p->BoxSize);
    StellarArgs sa;
    sa.Box = p->BoxSize;
    sa.DesNumNgb = p->DesNumNgb;
    sa.MaxDev = p->MaxNgbDeviation;
    sa.SPHWeighting = p->SPHWeighting;
    sa.rho_leaf = ctx->hsml_leaf.ptr;
    sa.starvol = d_starvol;
    sa.todo = ctx->s_todo.ptr;
    unsigned long long *nint = reinterpret_cast<unsigned long long *>(ctx->s_counters.ptr + 1);
    sa.hmax_tried = nint + 2;
    int niter = 0;
    SHQ_HIP(hipEventRecord(ctx->ev_begin[SHQ_T_SPH], st));
    SHQ_TRY(sph_redo_loop(ctx, d_queue, nq, "failed to converge the stellar density for %lld stars",
                          [&](const int32_t *cur, long long size, unsigned grid, long long ntasks) {
                              switch(p->DensityKernelType) {
                              case 1: sph_stellar_kernel<1><<<dim3(grid), dim3(256), 0, st>>>(a, cur, size, sa, nint, ctx->s_nlist2.ptr, ntasks); break;
                              case 2: sph_stellar_kernel<2><<<dim3(grid), dim3(256), 0, st>>>(a, cur, size, sa, nint, ctx->s_nlist2.ptr, ntasks); break;
                              default: sph_stellar_kernel<4><<<dim3(grid), dim3(256), 0, st>>>(a, cur, size, sa, nint, ctx->s_nlist2.ptr, ntasks); break;
                              }
                          },
                          &niter));
    SHQ_HIP(hipEventRecord(ctx->ev_end[SHQ_T_SPH], st));
    if(stats)
        SHQ_TRY(sph_fill_stats(ctx, stats, nq, niter, nint, true));
    return SHQ_OK;
}

/* ---- black-hole velocity dispersion: veldisp2.cpp:20-199 ----------------------------------------
 * BHVelDispLocalTreeWalk::ngbiter (:126-144): over the dark matter inside a black hole's Hsml, the count and the first and
 * second moments of the predicted DM velocity (KickFactorData::DM_VelPred, density2.h:104-111) relative to the hole's;
 * BHVelDispOutput::postprocess (:49-63) turns them into VDisp.  Same fused walk as the other neighbour operators; the tree is
 * the caller's dark-matter tree. */
struct BhVdArgs {
    const double4 *vel_leaf;  /* predicted DM velocity by leaf slot */
    const double *vel;        /* [N][3] raw velocities (the hole's own) */
    double *out;              /* [nq][5]: NumDM, V1sumDM[3], V2sumDM, by queue position */
};

__global__ __launch_bounds__(256) void bh_veldisp_kernel(const SphDev a, const int32_t *queue, long long nq, const BhVdArgs ba,
                                                         int32_t *__restrict__ nlist, long long ntasks)
{
    __shared__ __attribute__((aligned(32))) char lds[4 * NW_LDS_PER_WAVE(false)];
    const int lane = threadIdx.x & 63;
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = wave * 64 + lane;
    const bool valid = t < nq;
    double px = 0, py = 0, pz = 0, h = 1, vx = 0, vy = 0, vz = 0;
    if(valid) {
        const long long pi = queue[t];
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z;
        h = a.hsml[pi];
        vx = ba.vel[3 * pi]; vy = ba.vel[3 * pi + 1]; vz = ba.vel[3 * pi + 2];
    }
    const double h2 = h * h;
    double num = 0, s0 = 0, s1 = 0, s2 = 0, v2 = 0;
    auto pair = [&](const int s) {
        const double4 w = ba.vel_leaf[s];
        num += 1;
        const double e0 = w.x - vx, e1 = w.y - vy, e2 = w.z - vz;
        s0 += e0; v2 += e0 * e0;
        s1 += e1; v2 += e1 * e1;
        s2 += e2; v2 += e2 * e2;
    };
    auto accept = [&](const double r2, const double, const int) { return r2 > 0 && r2 < h2; };
    int fill = 0;
    bool ovf = false;
    (void) ngb_walk<false, false, false>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(false), myl, valid, px, py, pz, h, accept, pair,
                                         (unsigned int *) nullptr, fill, ovf);
    if(valid) {
        ba.out[5 * t] = num;
        ba.out[5 * t + 1] = s0;
        ba.out[5 * t + 2] = s1;
        ba.out[5 * t + 3] = s2;
        ba.out[5 * t + 4] = v2;
    }
    } /* task loop */
}

/* neighbour-side arrays of the DM tree in leaf order: DM_VelPred and the skip flag (garbage / not dark matter any more) */
__global__ void bh_veldisp_gather_kernel(long long nleaf, const int32_t *__restrict__ pidx, const double *__restrict__ vel,
                                         const double *__restrict__ treeacc, const double *__restrict__ gravpm, const uint8_t *__restrict__ bin_grav,
                                         const uint8_t *__restrict__ pflags, shq_kick_factors kf, int typemask, double4 *vel_leaf, int32_t *flag_leaf)
{
#pragma clang fp contract(off)
    const long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(s >= nleaf)
        return;
    const long long p = pidx[s];
    double v[3];
    for(int j = 0; j < 3; j++)
        v[j] = vel[3 * p + j] + kf.gravkicks[bin_grav[p]] * treeacc[3 * p + j] + gravpm[3 * p + j] * kf.FgravkickB;
    vel_leaf[s] = make_double4(v[0], v[1], v[2], 0.0);
    const unsigned f = pflags[p];
    flag_leaf[s] = ((f & 1u) || !((1 << (f >> 4)) & typemask)) ? 1 : 0;
}

int shq_bh_veldisp_device(shq_context *ctx, const shq_kick_factors *kf, double BoxSize, const int32_t *d_queue, int64_t nq, double *d_out)
{
    if(nq == 0)
        return SHQ_OK;
    const long long nl = ctx->ntreeparts + SHQ_NMAXCHILD;
    SHQ_TRY(ctx->velp_leaf.reserve(nl));
    SHQ_TRY(ctx->flag_leaf.reserve(nl));
    SHQ_TRY(sph_reserve_nlist2(ctx));
    hipStream_t st = ctx->stream;
    bh_veldisp_gather_kernel<<<dim3(nblk(nl)), dim3(256), 0, st>>>(nl, ctx->leaf_pidx.ptr, ctx->vel.ptr, ctx->treeacc.ptr, ctx->gravpm.ptr,
                                                                  ctx->bin_grav.ptr, ctx->pflags.ptr, *kf, 1 << 1, ctx->velp_leaf.ptr,
                                                                  ctx->flag_leaf.ptr);
    SHQ_HIP(hipGetLastError());
    SphDev a = make_dev(ctx, BoxSize);
    BhVdArgs ba;
    ba.vel_leaf = ctx->velp_leaf.ptr;
    ba.vel = ctx->vel.ptr;
    ba.out = d_out;
    const long long ntasks = (nq + 255) / 256;
    const unsigned grid = (unsigned) (ntasks < NL_REDO_BLOCKS ? ntasks : NL_REDO_BLOCKS);
    bh_veldisp_kernel<<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, ba, ctx->s_nlist2.ptr, ntasks);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* ---- wind velocity dispersion: winds_find_vel_disp, veldisp2.cpp:203-528 --------------------------
 * The 1-D velocity dispersion of the ~40 nearest dark-matter particles around star-forming gas: a density-like loop over the
 * DM tree with NWINDHSML = 5 trial radii per walk (vdispeffdmradius :216-229, ngbiter :440-479 with the Hubble flow in the
 * relative velocity), WindVDispOutput::postprocess + ngb_narrow_down (:285-320) until 40 +- 1 neighbours.  Same structure
 * as the stellar density; the reference's integer neighbour counts make the result independent of summation order. */
#define WV_NH 5
#define WV_NUMDMNGB 40
#define WV_MAXDEV 1

template <int NH> __device__ __forceinline__ double narrow_down(double &R, double &L, const double *radius, const double *numNgb, int maxcmpt,
                                                                 int desnumngb, int &close, double Box)
{
    /* ngb_narrow_down, treewalk.c:1349-1406, with the dynamic indices written as selects over the NH trial radii */
    close = 0;
    double ngbdist = fabs(numNgb[0] - desnumngb);
#pragma unroll
    for(int k = 1; k < NH; k++) {
        const double nd = fabs(numNgb[k] - desnumngb);
        if(k < maxcmpt && nd < ngbdist) {
            ngbdist = nd;
            close = k;
        }
    }
    bool stop = false;
#pragma unroll
    for(int k = 0; k < NH; k++) {
        if(k < maxcmpt && !stop) {
            if(numNgb[k] < desnumngb)
                L = radius[k];
            if(numNgb[k] > desnumngb) {
                R = radius[k];
                stop = true;
            }
        }
    }
    double hc = radius[0], rl = radius[0], rl1 = radius[0], nl = numNgb[0], nl1 = numNgb[0];
#pragma unroll
    for(int k = 1; k < NH; k++) {
        if(k == close)
            hc = radius[k];
        if(k == maxcmpt - 1) {
            rl = radius[k]; nl = numNgb[k]; rl1 = radius[k - 1]; nl1 = numNgb[k - 1];
        }
    }
    double hs = hc;
    if(R > 0.99 * Box) {
        double dngbdv = 0;
        if(maxcmpt > 1 && rl > rl1)
            dngbdv = (nl - nl1) / (pow(rl, 3) - pow(rl1, 3));
        double newh = 4 * hs;
        if(dngbdv > 0) {
            const double dngb = desnumngb - nl;
            const double nv = pow(hs, 3) + dngb / dngbdv;
            if(pow(nv, 1. / 3) < newh)
                newh = pow(nv, 1. / 3);
        }
        hs = newh;
    }
    if(hs > R)
        hs = R;
    if(L == 0) {
        double dngbdv = 0;
        if(radius[1] > radius[0])
            dngbdv = (numNgb[1] - numNgb[0]) / (pow(radius[1], 3) - pow(radius[0], 3));
        if(maxcmpt == 1 && radius[0] > 0)
            dngbdv = numNgb[0] / pow(radius[0], 3);
        if(dngbdv > 0) {
            const double dngb = desnumngb - numNgb[0];
            const double nv = pow(hs, 3) + dngb / dngbdv;
            hs = pow(nv, 1. / 3);
        }
    }
    if(hs < L)
        hs = L;
    return hs;
}

struct WindVdArgs {
    double Box, hubble_a2;     /* hubble * atime^2 */
    const double4 *vel_leaf;   /* DM_VelPred by leaf slot */
    const double *vel;         /* [N][3] */
    double *dmradius;          /* by particle index: the current DMRadius (starts as Hsml) */
    double *vdisp;             /* by particle index; < 0 where not set */
    int32_t *todo;
};

__global__ __launch_bounds__(256) void wind_veldisp_kernel(const SphDev a, const int32_t *queue, long long nq, const WindVdArgs wa,
                                                           unsigned long long *nint_total, int32_t *__restrict__ nlist, long long ntasks)
{
    __shared__ __attribute__((aligned(32))) char lds[4 * NW_LDS_PER_WAVE(false)];
    const int lane = threadIdx.x & 63;
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = wave * 64 + lane;
    const bool valid = t < nq;
    long long pi = 0;
    double px = 0, py = 0, pz = 0, vx = 0, vy = 0, vz = 0, dm = 1, L = 0, R = wa.Box;
    if(valid) {
        pi = queue[t];
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z;
        vx = wa.vel[3 * pi]; vy = wa.vel[3 * pi + 1]; vz = wa.vel[3 * pi + 2];
        dm = wa.dmradius[pi];
        L = a.left[pi];
        R = a.right[pi];
    }
    double rad[WV_NH], num[WV_NH], v1x[WV_NH], v1y[WV_NH], v1z[WV_NH], v2[WV_NH];
    {
        /* vdispeffdmradius, veldisp2.cpp:216-229 */
        double right = R, left = L;
        if(right > 0.99 * wa.Box)
            right = dm;
        if(left == 0)
            left = 0.1 * dm;
        const double rvol = pow(right, 3), lvol = pow(left, 3);
#pragma unroll
        for(int k = 0; k < WV_NH; k++) {
            rad[k] = pow((1.0 * k + 1) / (1.0 * WV_NH + 1) * (rvol - lvol) + lvol, 1. / 3);
            num[k] = 0; v1x[k] = 0; v1y[k] = 0; v1z[k] = 0; v2[k] = 0;
        }
    }
    int maxcmpte = WV_NH;
    auto pair = [&](const int s) {
        const double4 q = a.posm_leaf[s];
        const double4 w = wa.vel_leaf[s];
        const double d0 = wrapd(px - q.x, a.Box, a.invBox);
        const double d1 = wrapd(py - q.y, a.Box, a.invBox);
        const double d2 = wrapd(pz - q.z, a.Box, a.invBox);
        const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
        if(r2 <= 0 || !(r2 < rad[WV_NH - 1] * rad[WV_NH - 1]))
            return;
        const double r = sqrt(r2);
        const double e0 = w.x - vx + wa.hubble_a2 * d0, e1 = w.y - vy + wa.hubble_a2 * d1, e2 = w.z - vz + wa.hubble_a2 * d2;
#pragma unroll
        for(int k = 0; k < WV_NH; k++) {
            if(k < maxcmpte && r < rad[k]) {
                num[k] += 1;
                v1x[k] += e0; v2[k] += e0 * e0;
                v1y[k] += e1; v2[k] += e1 * e1;
                v1z[k] += e2; v2[k] += e2 * e2;
            }
        }
        int first = WV_NH;
#pragma unroll
        for(int k = WV_NH - 1; k >= 0; k--)
            first = (num[k] > WV_NUMDMNGB) ? k : first;
        if(first < WV_NH)
            maxcmpte = first + 1;
    };
    const double rw2 = rad[WV_NH - 1] * rad[WV_NH - 1];
    auto accept = [&](const double r2, const double, const int) { return r2 > 0 && r2 < rw2; };
    int fill = 0;
    bool ovf = false;
    unsigned int nint = ngb_walk<false, false, false>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(false), myl, valid, px, py, pz, rad[WV_NH - 1],
                                                      accept, pair, (unsigned int *) nullptr, fill, ovf);
    if(valid) {
        /* WindVDispOutput::postprocess, veldisp2.cpp:285-320 */
        int close = 0;
        const double newdm = narrow_down<WV_NH>(R, L, rad, num, maxcmpte, WV_NUMDMNGB, close, wa.Box);
        double nc = num[0], s0 = v1x[0], s1 = v1y[0], s2 = v1z[0], q2 = v2[0];
#pragma unroll
        for(int k = 1; k < WV_NH; k++)
            if(k == close) {
                nc = num[k]; s0 = v1x[k]; s1 = v1y[k]; s2 = v1z[k]; q2 = v2[k];
            }
        wa.dmradius[pi] = newdm;
        a.left[pi] = L;
        a.right[pi] = R;
        a.numngb[pi] = nc;
        int done = 0;
        if((nc >= (WV_NUMDMNGB - WV_MAXDEV) && nc <= (WV_NUMDMNGB + WV_MAXDEV)) || (R - L < 5e-6 * L)) {
            double vd = q2 / nc;
            vd -= (s0 / nc) * (s0 / nc);
            vd -= (s1 / nc) * (s1 / nc);
            vd -= (s2 / nc) * (s2 / nc);
            if(vd > 0)
                wa.vdisp[pi] = sqrt(vd / 3);
            done = 1;
        }
        wa.todo[t] = done ? -1 : (int32_t) pi;
    }
    unsigned int sn = nint;
    for(int off = 32; off > 0; off >>= 1)
        sn += __shfl_xor(sn, off);
    if(lane == 0 && nint_total)
        atomicAdd(nint_total, (unsigned long long) sn);
    } /* task loop */
}

int shq_wind_veldisp_device(shq_context *ctx, const shq_kick_factors *kf, double BoxSize, double hubble_a2, const int32_t *d_queue, int64_t nq,
                            double *d_dmradius, double *d_vdisp, shq_sph_stats *stats)
{
    const long long n = ctx->numpart;
    SHQ_TRY(sph_reserve_redo(ctx));
    SHQ_TRY(sph_reserve_nlist2(ctx));
    const long long nl = ctx->ntreeparts + SHQ_NMAXCHILD;
    SHQ_TRY(ctx->velp_leaf.reserve(nl));
    SHQ_TRY(ctx->flag_leaf.reserve(nl));
    hipStream_t st = ctx->stream;
    if(n > 0) {
        SHQ_HIP(hipMemsetAsync(ctx->s_left.ptr, 0, sizeof(double) * n, st));
        sph_fill(ctx, ctx->s_right.ptr, n, BoxSize);
    }
    SHQ_HIP(hipMemsetAsync(ctx->s_counters.ptr, 0, sizeof(long long) * 8, st));
    bh_veldisp_gather_kernel<<<dim3(nblk(nl)), dim3(256), 0, st>>>(nl, ctx->leaf_pidx.ptr, ctx->vel.ptr, ctx->treeacc.ptr, ctx->gravpm.ptr,
                                                                  ctx->bin_grav.ptr, ctx->pflags.ptr, *kf, 1 << 1, ctx->velp_leaf.ptr,
                                                                  ctx->flag_leaf.ptr);
    SHQ_HIP(hipGetLastError());
    SphDev a = make_dev(ctx, BoxSize);
    WindVdArgs wa;
    wa.Box = BoxSize;
    wa.hubble_a2 = hubble_a2;
    wa.vel_leaf = ctx->velp_leaf.ptr;
    wa.vel = ctx->vel.ptr;
    wa.dmradius = d_dmradius;
    wa.vdisp = d_vdisp;
    wa.todo = ctx->s_todo.ptr;
    unsigned long long *nint = reinterpret_cast<unsigned long long *>(ctx->s_counters.ptr + 1);
    int niter = 0;
    SHQ_HIP(hipEventRecord(ctx->ev_begin[SHQ_T_SPH], st));
    SHQ_TRY(sph_redo_loop(ctx, d_queue, nq, "failed to converge the wind velocity dispersion for %lld particles",
                          [&](const int32_t *cur, long long size, unsigned grid, long long ntasks) {
                              wind_veldisp_kernel<<<dim3(grid), dim3(256), 0, st>>>(a, cur, size, wa, nint, ctx->s_nlist2.ptr, ntasks);
                          },
                          &niter));
    SHQ_HIP(hipEventRecord(ctx->ev_end[SHQ_T_SPH], st));
    if(stats)
        SHQ_TRY(sph_fill_stats(ctx, stats, nq, niter, nint));
    return SHQ_OK;
}

/* ---- black-hole repositioning and dynamical-friction sums: bhdynfric.cpp:44-295 --------------------
 * BHReposLocalTreeWalk::ngbiter (:160-174): the particle of lowest potential inside the hole's kernel radius (position and
 * velocity kept; first one met in depth-first order on ties).  BHDynFricLocalTreeWalk::ngbiter (:193-224): the same plus the
 * kernel-weighted mass, momentum (DM_VelPred) and squared velocity of the surrounding stars (and dark matter for method > 1).
 * BHDynFricOutput::postprocess (:66-82) normalises.  The tree (ALLMASK, or STARMASK + BHMASK [+ DMMASK]) is the caller's. */
struct BhDfArgs {
    const double4 *vp_leaf;    /* DM_VelPred, weight: 1 if the particle counts for the friction sums */
    const double4 *rv_leaf;    /* raw Vel, Potential */
    double *out;               /* [nq][12]: MinPot, MinPotPos[3], MinPotVel[3], Density, Vel[3], RmsVel (raw sums) */
    int dosums;
};

template <int KT>
__global__ __launch_bounds__(256) void bh_dynfric_kernel(const SphDev a, const int32_t *queue, long long nq, const BhDfArgs da,
                                                         int32_t *__restrict__ nlist, long long ntasks)
{
    __shared__ __attribute__((aligned(32))) char lds[4 * NW_LDS_PER_WAVE(false)];
    const int lane = threadIdx.x & 63;
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = wave * 64 + lane;
    const bool valid = t < nq;
    double px = 0, py = 0, pz = 0, h = 1;
    if(valid) {
        const long long pi = queue[t];
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z;
        h = a.hsml[pi];
    }
    const Kern<KT> kernel(h);
    const double h2 = kernel.H * kernel.H, Hinv = 1.0 / kernel.H;
    double minpot = 1.0e29 /* BHPOTVALUEINIT */, mp0 = -1, mp1 = -1, mp2 = -1, mv0 = 0, mv1 = 0, mv2 = 0;
    double dens = 0, sv0 = 0, sv1 = 0, sv2 = 0, rms = 0;
    auto pair = [&](const int s) {
        const double4 q = a.posm_leaf[s];
        const double4 rv = da.rv_leaf[s];
        if(rv.w < minpot) {
            minpot = rv.w;
            mp0 = q.x; mp1 = q.y; mp2 = q.z;
            mv0 = rv.x; mv1 = rv.y; mv2 = rv.z;
        }
        if(da.dosums) {
            const double4 vp = da.vp_leaf[s];
            if(vp.w != 0) {
                const double d0 = wrapd(px - q.x, a.Box, a.invBox), d1 = wrapd(py - q.y, a.Box, a.invBox), d2 = wrapd(pz - q.z, a.Box, a.invBox);
                const double u = sqrt(d0 * d0 + d1 * d1 + d2 * d2) * Hinv;
                const double mw = q.w * kernel.wk(u);
                dens += mw;
                sv0 += mw * vp.x; rms += mw * (vp.x * vp.x);
                sv1 += mw * vp.y; rms += mw * (vp.y * vp.y);
                sv2 += mw * vp.z; rms += mw * (vp.z * vp.z);
            }
        }
    };
    auto accept = [&](const double r2, const double, const int) { return r2 < h2; };
    int fill = 0;
    bool ovf = false;
    (void) ngb_walk<false, false, false>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(false), myl, valid, px, py, pz, kernel.H, accept, pair,
                                         (unsigned int *) nullptr, fill, ovf);
    if(valid) {
        double *o = da.out + 12 * t;
        o[0] = minpot; o[1] = mp0; o[2] = mp1; o[3] = mp2; o[4] = mv0; o[5] = mv1; o[6] = mv2;
        o[7] = dens; o[8] = sv0; o[9] = sv1; o[10] = sv2; o[11] = rms;
    }
    } /* task loop */
}

__global__ void bh_dynfric_gather_kernel(long long nleaf, const int32_t *__restrict__ pidx, const double *__restrict__ vel,
                                         const double *__restrict__ treeacc, const double *__restrict__ gravpm, const uint8_t *__restrict__ bin_grav,
                                         const uint8_t *__restrict__ pflags, const double *__restrict__ potential, shq_kick_factors kf,
                                         int typemask, int method, double4 *vp_leaf, double4 *rv_leaf, int32_t *flag_leaf)
{
#pragma clang fp contract(off)
    const long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(s >= nleaf)
        return;
    const long long p = pidx[s];
    double v[3];
    for(int j = 0; j < 3; j++)
        v[j] = vel[3 * p + j] + kf.gravkicks[bin_grav[p]] * treeacc[3 * p + j] + gravpm[3 * p + j] * kf.FgravkickB;
    const unsigned f = pflags[p];
    const int type = f >> 4;
    vp_leaf[s] = make_double4(v[0], v[1], v[2], (type == 4 || (type == 1 && method > 1)) ? 1.0 : 0.0);
    rv_leaf[s] = make_double4(vel[3 * p], vel[3 * p + 1], vel[3 * p + 2], potential[p]);
    flag_leaf[s] = ((f & 1u) || !((1 << type) & typemask)) ? 1 : 0;
}

int shq_bh_dynfric_device(shq_context *ctx, const shq_kick_factors *kf, double BoxSize, int kernel_type, int typemask, int method,
                          const double *d_potential, const int32_t *d_queue, int64_t nq, double *d_out)
{
    if(nq == 0)
        return SHQ_OK;
    SHQ_CHECK(kernel_type == 1 || kernel_type == 2 || kernel_type == 4, SHQ_ERR_INVALID, "unknown DensityKernelType %d", kernel_type);
    const long long nl = ctx->ntreeparts + SHQ_NMAXCHILD;
    SHQ_TRY(ctx->velp_leaf.reserve(nl));
    SHQ_TRY(ctx->hydrec_leaf.reserve((size_t) nl * sizeof(double4) + 128)); /* reused for the raw velocity + potential stream */
    SHQ_TRY(ctx->flag_leaf.reserve(nl));
    SHQ_TRY(sph_reserve_nlist2(ctx));
    hipStream_t st = ctx->stream;
    double4 *rv_leaf = reinterpret_cast<double4 *>(ctx->hydrec_leaf.ptr);
    bh_dynfric_gather_kernel<<<dim3(nblk(nl)), dim3(256), 0, st>>>(nl, ctx->leaf_pidx.ptr, ctx->vel.ptr, ctx->treeacc.ptr, ctx->gravpm.ptr,
                                                                  ctx->bin_grav.ptr, ctx->pflags.ptr, d_potential, *kf, typemask, method,
                                                                  ctx->velp_leaf.ptr, rv_leaf, ctx->flag_leaf.ptr);
    SHQ_HIP(hipGetLastError());
    SphDev a = make_dev(ctx, BoxSize);
    BhDfArgs da;
    da.vp_leaf = ctx->velp_leaf.ptr;
    da.rv_leaf = rv_leaf;
    da.out = d_out;
    da.dosums = method > 0;
    const long long ntasks = (nq + 255) / 256;
    const unsigned grid = (unsigned) (ntasks < NL_REDO_BLOCKS ? ntasks : NL_REDO_BLOCKS);
    switch(kernel_type) {
    case 1: bh_dynfric_kernel<1><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, da, ctx->s_nlist2.ptr, ntasks); break;
    case 2: bh_dynfric_kernel<2><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, da, ctx->s_nlist2.ptr, ntasks); break;
    default: bh_dynfric_kernel<4><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, da, ctx->s_nlist2.ptr, ntasks); break;
    }
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

namespace {
__global__ void gradmag_kernel(const double *g, double *out, long long n)
{
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n)
        out[i] = sqrt(g[3 * i] * g[3 * i] + g[3 * i + 1] * g[3 * i + 1] + g[3 * i + 2] * g[3 * i + 2]);
}
} // namespace

int shq_sph_gradrho_mag(shq_context *ctx, double *d_out)
{
    const long long n = ctx->numpart;
    if(n > 0)
        gradmag_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(ctx->s_gradrho.ptr, d_out, n);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}
