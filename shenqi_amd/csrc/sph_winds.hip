/* sph_winds.hip — stellar winds from new stars (walk, nearest-star resolution, kick), metal return around dying stars, and the
 * wind model's particle loops, on the walk of sph_walk.hpp. */
#include "sph_walk.hpp"
#include "device_prims.hpp"
#include <utility>

/* ---- stellar winds from new stars: libgadget/winds.cpp:227-369, 411-447, 510-565 --------------------------
 * Two asymmetric legacy-API walks over the gas tree for the new stars of the step: the total mass of the gas inside the star's
 * Hsml that is not already a wind particle (sfr_wind_weight_ngbiter), then the kick candidates: every such gas particle whose
 * draw Table[(star ID + gas ID) % size] falls below windeff * Mass / TotalWeight is appended to one list of (gas particle, distance,
 * star ID, velocity, thermal energy) — sfr_wind_feedback_ngbiter's StarKick queue.  Which candidate kicks (the nearest star, ties to
 * the smaller star ID) is resolved from the sorted list by the caller of these kernels, as the reference does after its walk. */
__global__ void wind_gather_leaf_kernel(long long nleaf, const int32_t *__restrict__ pidx, const uint8_t *__restrict__ pflags, const double *__restrict__ delay,
                                        int32_t *flag_leaf)
{
    const long long s = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(s >= nleaf)
        return;
    const int p = pidx[s];
    const unsigned f = pflags[p];
    flag_leaf[s] = ((f & 3u) || (f >> 4) != 0 || delay[p] > 0) ? 1 : 0; /* GASMASK, garbage, "skip earlier wind particles" */
}

template <bool KICK>
__global__ __launch_bounds__(256) void wind_walk_kernel(const SphDev a, const int32_t *queue, long long nq, const WindWalkArgs w, int32_t *__restrict__ nlist,
                                                        long long ntasks)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(32))) char lds[4 * NW_LDS_PER_WAVE(false)];
    const int lane = threadIdx.x & 63;
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = wave * 64 + lane;
    const bool valid = t < nq;
    double px = 0, py = 0, pz = 0, h = 1, imass = 0, tw = 0, vdisp = 0;
    unsigned long long myid = 0;
    if(valid) {
        const long long pi = queue[t];
        const double4 p = a.posm[pi];
        px = p.x; py = p.y; pz = p.z;
        imass = p.w;
        h = a.hsml[pi];
        if(KICK) {
            myid = w.ids[pi];
            tw = w.totalweight[t];
            vdisp = w.vdisp[t];
        }
    }
    const double h2 = h * h;
    /* get_wind_params, winds.cpp:489-507 */
    double vel = 0, windeff = 0, utherm = 0;
    if(KICK) {
        const double vphys = vdisp / w.P.Time;
        utherm = w.P.WindThermalFactor * 1.5 * vphys * vphys;
        if(w.P.WindModel & 8) {
            windeff = w.P.WindEfficiency;
            vel = w.P.WindSpeed * w.P.Time;
        } else {
            windeff = (w.P.WindSigma0 * w.P.WindSigma0) / (vphys * vphys + 2 * utherm);
            vel = w.P.WindSpeedFactor * vdisp;
        }
        if(vel < w.P.MinWindVelocity * w.P.Time)
            vel = w.P.MinWindVelocity * w.P.Time;
    }
    double sum = 0;
    unsigned int visited = 0;
    auto pair = [&](const int s) {
        const double4 q = a.posm_leaf[s];
        const double d0 = wrapd(px - q.x, a.Box, a.invBox), d1 = wrapd(py - q.y, a.Box, a.invBox), d2 = wrapd(pz - q.z, a.Box, a.invBox);
        const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if(r > h)
            return;
        if(!KICK) {
            sum += q.w; /* wk = 1 */
            visited++;
            return;
        }
        if(tw == 0 || vdisp <= 0)
            return;
        const long long p = w.leaf_pidx[s];
        const double prob = windeff * imass / tw;
        const double rn = w.rnd[(myid + w.ids[p]) % w.rndsize];
        if(rn < prob && vel > 0) {
            const unsigned long long k = atomicAdd(w.nkicks, 1ull);
            if(k < w.maxkicks) {
                shq_wind_kick &K = w.kicks[k];
                K.part_index = (int32_t) p;
                K.pad_ = 0;
                K.StarDistance = r;
                K.StarID = myid;
                K.StarKickVelocity = vel;
                K.StarTherm = utherm;
            }
        }
    };
    auto accept = [&](const double r2, const double, const int) { return r2 <= h2; };
    int fill = 0;
    bool ovf = false;
    (void) ngb_walk<false, false, false>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(false), myl, valid, px, py, pz, h, accept, pair,
                                         (unsigned int *) nullptr, fill, ovf);
    if(!KICK) {
        if(valid)
            w.totalweight[t] = sum;
        for(int off = 32; off > 0; off >>= 1)
            visited += __shfl_xor(visited, off);
        if(lane == 0 && visited)
            atomicAdd(w.nvisited, (unsigned long long) visited);
    }
    } /* task loop */
}

/* the StarKick resolution (winds.cpp:330-350) on the device: the candidates sorted by (particle, distance, star ID) — three stable
 * radix sorts, least significant key first — then the first candidate of every particle kicks: wind_do_kick + get_wind_dir, :449-487 */
__global__ void wind_kick_keys_kernel(long long n, const shq_wind_kick *k, int which, unsigned long long *keys, int32_t *idx, const int32_t *order)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= n)
        return;
    const int32_t j = order ? order[t] : (int32_t) t;
    const shq_wind_kick &K = k[j];
    keys[t] = which == 0 ? K.StarID : (which == 1 ? (unsigned long long) __double_as_longlong(K.StarDistance) /* >= 0: bits order like values */
                                                   : (unsigned long long) (unsigned) K.part_index);
    idx[t] = j;
}

__global__ void wind_kick_gather_kernel(long long n, const shq_wind_kick *k, const int32_t *order, shq_wind_kick *out)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t < n)
        out[t] = k[order[t]];
}

__global__ void wind_do_kick_kernel(long long n, const shq_wind_kick *k, const WindWalkArgs w, double *vel, double *entropy, const double *density, double *delay,
                                    unsigned long long *napplied, int *odd)
{
#pragma clang fp contract(off)
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= n)
        return;
    const shq_wind_kick K = k[t];
    if(t > 0 && k[t - 1].part_index == K.part_index)
        return; /* "Only do the kick for the first particle, which is the closest" */
    const long long other = K.part_index;
    const unsigned long long id = w.ids[other];
    const double theta = acos(2 * w.rnd[(id + 3) % w.rndsize] - 1);
    const double phi = 2 * M_PI * w.rnd[(id + 4) % w.rndsize];
    const double dir[3] = {sin(theta) * cos(phi), sin(theta) * sin(phi), cos(theta)};
    const double v = K.StarKickVelocity, atime = w.P.Time;
    if(v > 0 && atime > 0) {
        for(int j = 0; j < 3; j++)
            vel[3 * other + j] += v * dir[j];
        const double enttou = pow(density[other] / pow(atime, 3), SPH_GAMMA_MINUS1) / SPH_GAMMA_MINUS1;
        entropy[other] += K.StarTherm / enttou;
        if((w.P.WindModel & 2) && w.P.MaxWindFreeTravelTime > 0) { /* winds_ever_decouple */
            double d = w.P.WindFreeTravelLength / (v / atime);
            if(d > w.P.MaxWindFreeTravelTime)
                d = w.P.MaxWindFreeTravelTime;
            delay[other] = d;
        }
    }
    if(!(v > 0) || !isfinite(v) || !isfinite(delay[other]))
        *odd = 1; /* "Odd v", winds.cpp:344 */
    atomicAdd(napplied, 1ull);
}

int shq_wind_resolve_device(shq_context *ctx, const WindWalkArgs *w, long long nk, shq_wind_kick *d_sorted, unsigned long long *d_napplied, int *d_odd, bool apply)
{
    if(nk == 0)
        return SHQ_OK;
    hipStream_t st = ctx->stream;
    SHQ_TRY(ctx->metal_keys[0].reserve((size_t) nk));
    SHQ_TRY(ctx->metal_keys[1].reserve((size_t) nk));
    SHQ_TRY(ctx->s_queue2.reserve((size_t) nk));
    SHQ_TRY(ctx->s_queue3.reserve((size_t) nk));
    int32_t *ord[2] = {ctx->s_queue2.ptr, ctx->s_queue3.ptr};
    const int32_t *cur = nullptr;
    for(int which = 0; which < 3; which++) {
        wind_kick_keys_kernel<<<dim3(nblk(nk)), dim3(256), 0, st>>>(nk, w->kicks, which, ctx->metal_keys[0].ptr, ord[0], cur);
        SHQ_HIP(hipGetLastError());
        SHQ_TRY(prim_sort_pairs(ctx, ctx->metal_keys[0].ptr, ctx->metal_keys[1].ptr, ord[0], ord[1], (size_t) nk, 0, 64));
        cur = ord[1];
        std::swap(ord[0], ord[1]); /* the next pass writes its identity-permuted indices over the old input */
    }
    wind_kick_gather_kernel<<<dim3(nblk(nk)), dim3(256), 0, st>>>(nk, w->kicks, cur, d_sorted);
    SHQ_HIP(hipGetLastError());
    if(apply) {
        wind_do_kick_kernel<<<dim3(nblk(nk)), dim3(256), 0, st>>>(nk, d_sorted, *w, ctx->vel.ptr, ctx->g_entropy.ptr, ctx->g_density.ptr, ctx->g_delaytime.ptr, d_napplied,
                                                                  d_odd);
        SHQ_HIP(hipGetLastError());
    }
    return SHQ_OK;
}

int shq_wind_walk_device(shq_context *ctx, const WindWalkArgs *w, const int32_t *d_queue, int64_t nq, bool kick)
{
    if(nq == 0)
        return SHQ_OK;
    hipStream_t st = ctx->stream;
    const long long nl = ctx->ntreeparts + SHQ_NMAXCHILD;
    SHQ_TRY(ctx->flag_leaf.reserve(nl));
    wind_gather_leaf_kernel<<<dim3(nblk(nl)), dim3(256), 0, st>>>(nl, ctx->leaf_pidx.ptr, ctx->pflags.ptr, ctx->g_delaytime.ptr, ctx->flag_leaf.ptr);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(sph_reserve_nlist2(ctx));
    SphDev a = make_dev(ctx, w->P.BoxSize);
    const long long ntasks = (nq + 255) / 256;
    const unsigned grid = (unsigned) (ntasks < NL_REDO_BLOCKS ? ntasks : NL_REDO_BLOCKS);
    if(kick)
        wind_walk_kernel<true><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, ctx->s_nlist2.ptr, ntasks);
    else
        wind_walk_kernel<false><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, ctx->s_nlist2.ptr, ntasks);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* ---- metal return to the gas around dying stars: libgadget/metal_return.cpp:582-667 -----------------------
 * metal_return_ngbiter updates every gas particle inside a star's kernel under a per-particle spin lock: the result depends on the
 * order the stars reach a particle in (float mass, the MaxGasMass cut).  Here the walk (one star per lane, asymmetric, gas tree) only
 * EMITS (gas particle, star, wk) triples; they are sorted by (particle, position of the star in the queue) and one thread per gas
 * particle applies its triples in that order with the reference's arithmetic — the serial loop over the queue, deterministic.  The
 * mass each star gave away is then summed per star in particle order. */
template <int KT, bool EMIT>
__global__ __launch_bounds__(256) void metal_emit_kernel(const SphDev a, const int32_t *queue, long long nq, const MetalWalkArgs w, int32_t *__restrict__ nlist,
                                                         long long ntasks)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(32))) char lds[4 * NW_LDS_PER_WAVE(false)];
    const int lane = threadIdx.x & 63;
    for(long long task = xcd_block(blockIdx.x, gridDim.x); task < ntasks; task += gridDim.x) {
    const long long wave = task * (blockDim.x >> 6) + (threadIdx.x >> 6);
    int32_t *myl = nlist + ((size_t) blockIdx.x * 4 + (threadIdx.x >> 6)) * (size_t) (NL_ROWS * 64) + lane;
    const long long t = wave * 64 + lane;
    const bool valid = t < nq;
    double px = 0, py = 0, pz = 0, h = 1;
    if(valid) {
        const double4 p = a.posm[queue[t]];
        px = p.x; py = p.y; pz = p.z;
        h = a.hsml[queue[t]];
    }
    const Kern<KT> kernel(h);
    const double HH = kernel.H * kernel.H, Hinv = 1.0 / kernel.H;
    unsigned int mine = 0;
    auto pair = [&](const int s) {
        if(!EMIT) {
            mine++;
            return;
        }
        const double4 q = a.posm_leaf[s];
        const double d0 = wrapd(px - q.x, a.Box, a.invBox), d1 = wrapd(py - q.y, a.Box, a.invBox), d2 = wrapd(pz - q.z, a.Box, a.invBox);
        const double r = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        double wk = 1;
        if(w.SPHWeighting)
            wk = kernel.wk(r * Hinv);
        const unsigned long long k = atomicAdd(w.cursor, 1ull);
        if(k < w.capacity) {
            w.keys[k] = ((unsigned long long) (unsigned) w.leaf_pidx[s] << 32) | (unsigned long long) t;
            w.wk[k] = wk;
        }
    };
    auto accept = [&](const double r2, const double, const int) { return r2 > 0 && r2 < HH; };
    int fill = 0;
    bool ovf = false;
    (void) ngb_walk<false, false, false>(a, lds + (threadIdx.x >> 6) * NW_LDS_PER_WAVE(false), myl, valid, px, py, pz, h, accept, pair,
                                         (unsigned int *) nullptr, fill, ovf);
    if(!EMIT) {
        for(int off = 32; off > 0; off >>= 1)
            mine += __shfl_xor(mine, off);
        if(lane == 0 && mine)
            atomicAdd(w.cursor, (unsigned long long) mine);
    }
    } /* task loop */
}

/* one thread per run of equal gas particles in the (particle, star)-sorted list: metal_return_ngbiter's body, :622-660 */
/* ord (may be NULL: the list itself is sorted): wk and thismass_out are indexed by ord[k], the place of sorted pair k in the caller's list */
__global__ void metal_apply_kernel(long long npairs, const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ ord, const double *__restrict__ wk,
                                   const MetalWalkArgs w, double *thismass_out)
{
#pragma clang fp contract(off)
    const long long k0 = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k0 >= npairs)
        return;
    const unsigned p = (unsigned) (keys[k0] >> 32);
    if(k0 > 0 && (unsigned) (keys[k0 - 1] >> 32) == p)
        return;
    float mass = w.gmass[p];
    double density = w.gdensity[p], metallicity = w.gmetallicity[p];
    float metals[SHQ_NMETALS];
    for(int i = 0; i < SHQ_NMETALS; i++)
        metals[i] = w.gmetals[(size_t) p * SHQ_NMETALS + i];
    for(long long k = k0; k < npairs && (unsigned) (keys[k] >> 32) == p; k++) {
        const unsigned t = (unsigned) (keys[k] & 0xffffffffull);
        const size_t j = ord ? (size_t) ord[k] : (size_t) k, ts = (size_t) t * w.star_stride;
        const double volume = mass / density;
        const double returnfraction = wk[j] * volume / w.starvolume[ts];
        const double thismass = returnfraction * w.massgenerated[ts];
        if(mass + thismass > w.MaxGasMass) {
            thismass_out[j] = 0;
            continue;
        }
        for(int i = 0; i < SHQ_NMETALS; i++) {
            const double tm = returnfraction * w.speciesgenerated[(size_t) t * w.species_stride + i];
            metals[i] = (float) ((metals[i] * mass + tm) / (mass + thismass));
        }
        const double thismetal = returnfraction * w.metalgenerated[ts];
        metallicity = (metallicity * mass + thismetal) / (mass + thismass);
        const double massfrac = (mass + thismass) / mass;
        mass = (float) (mass * massfrac);
        density *= massfrac;
        thismass_out[j] = thismass;
    }
    w.gmass[p] = mass;
    w.gdensity[p] = density;
    w.gmetallicity[p] = metallicity;
    for(int i = 0; i < SHQ_NMETALS; i++)
        w.gmetals[(size_t) p * SHQ_NMETALS + i] = metals[i];
    if(w.touched)
        w.touched[p] = 1;
}

__global__ void metal_rows_gather_kernel(long long m, const int32_t *__restrict__ list, const MetalWalkArgs w, double *rows)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= m)
        return;
    const size_t p = (size_t) list[t];
    double *r = rows + (size_t) (3 + SHQ_NMETALS) * t;
    r[0] = (double) w.gmass[p];
    r[1] = w.gdensity[p];
    r[2] = w.gmetallicity[p];
    for(int i = 0; i < SHQ_NMETALS; i++)
        r[3 + i] = (double) w.gmetals[p * SHQ_NMETALS + i];
}

__global__ void metal_rekey_kernel(long long npairs, const unsigned long long *keys, unsigned long long *out)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k < npairs)
        out[k] = (keys[k] << 32) | (keys[k] >> 32); /* (star, particle) */
}

/* O->MassReturn += thismass over a star's neighbours, in particle order */
__global__ void metal_sum_kernel(long long npairs, const unsigned long long *__restrict__ keys_tp, const double *__restrict__ thismass, double *massreturn)
{
#pragma clang fp contract(off)
    const long long k0 = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k0 >= npairs)
        return;
    const unsigned t = (unsigned) (keys_tp[k0] >> 32);
    if(k0 > 0 && (unsigned) (keys_tp[k0 - 1] >> 32) == t)
        return;
    double s = 0;
    for(long long k = k0; k < npairs && (unsigned) (keys_tp[k] >> 32) == t; k++)
        s += thismass[k];
    massreturn[t] = s;
}

int shq_metal_rows_gather(shq_context *ctx, const MetalWalkArgs *w, const int32_t *d_list, int64_t m, double *d_rows)
{
    if(m <= 0)
        return SHQ_OK;
    metal_rows_gather_kernel<<<dim3(nblk(m)), dim3(256), 0, ctx->stream>>>(m, d_list, *w, d_rows);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* the two emit passes: *np triples, (particle << 32 | queue position) in metal_keys[0] and wk in metal_val[0], in no particular order;
 * both pairs of buffers hold *np entries on return */
static int metal_emit_device(shq_context *ctx, MetalWalkArgs *w, int kernel_type, double BoxSize, const int32_t *d_queue, int64_t nq, unsigned long long *np_out)
{
    SHQ_CHECK(kernel_type == 1 || kernel_type == 2 || kernel_type == 4, SHQ_ERR_INVALID, "unknown DensityKernelType %d", kernel_type);
    hipStream_t st = ctx->stream;
    const long long nl = ctx->ntreeparts + SHQ_NMAXCHILD;
    SHQ_TRY(ctx->flag_leaf.reserve(nl));
    /* GASMASK, not garbage; wind particles take metals like any other gas */
    SHQ_TRY(sph_gather_gas_flags(ctx));
    SHQ_TRY(sph_reserve_nlist2(ctx));
    SHQ_TRY(ctx->wind_cnt.reserve(4));
    SphDev a = make_dev(ctx, BoxSize);
    const long long ntasks = (nq + 255) / 256;
    const unsigned grid = (unsigned) (ntasks < NL_REDO_BLOCKS ? ntasks : NL_REDO_BLOCKS);
    w->cursor = ctx->wind_cnt.ptr;
    w->leaf_pidx = ctx->leaf_pidx.ptr;
    unsigned long long np = 0;
    for(int pass = 0; pass < 2; pass++) {
        SHQ_HIP(hipMemsetAsync(ctx->wind_cnt.ptr, 0, sizeof(unsigned long long), st));
        if(pass == 0) {
            switch(kernel_type) {
            case 1: metal_emit_kernel<1, false><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, ctx->s_nlist2.ptr, ntasks); break;
            case 2: metal_emit_kernel<2, false><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, ctx->s_nlist2.ptr, ntasks); break;
            default: metal_emit_kernel<4, false><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, ctx->s_nlist2.ptr, ntasks); break;
            }
        } else {
            switch(kernel_type) {
            case 1: metal_emit_kernel<1, true><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, ctx->s_nlist2.ptr, ntasks); break;
            case 2: metal_emit_kernel<2, true><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, ctx->s_nlist2.ptr, ntasks); break;
            default: metal_emit_kernel<4, true><<<dim3(grid), dim3(256), 0, st>>>(a, d_queue, nq, *w, ctx->s_nlist2.ptr, ntasks); break;
            }
        }
        SHQ_HIP(hipGetLastError());
        unsigned long long h = 0;
        SHQ_HIP(hipMemcpyAsync(&h, ctx->wind_cnt.ptr, sizeof(h), hipMemcpyDeviceToHost, st));
        SHQ_HIP(hipStreamSynchronize(st));
        if(pass == 0) {
            np = h;
            if(np == 0)
                break;
            SHQ_TRY(ctx->metal_keys[0].reserve((size_t) np));
            SHQ_TRY(ctx->metal_keys[1].reserve((size_t) np));
            SHQ_TRY(ctx->metal_val[0].reserve((size_t) np));
            SHQ_TRY(ctx->metal_val[1].reserve((size_t) np));
            w->keys = ctx->metal_keys[0].ptr;
            w->wk = ctx->metal_val[0].ptr;
            w->capacity = np;
        } else
            SHQ_CHECK(h == np, SHQ_ERR_STATE, "metal_return: the two walks disagree on the number of pairs (%llu, %llu)", np, h);
    }
    *np_out = np;
    return SHQ_OK;
}

int shq_metal_return_device(shq_context *ctx, MetalWalkArgs *w, int kernel_type, double BoxSize, const int32_t *d_queue, int64_t nq, double *d_massreturn, int64_t *npairs_out)
{
    if(npairs_out)
        *npairs_out = 0;
    if(nq == 0)
        return SHQ_OK;
    hipStream_t st = ctx->stream;
    unsigned long long np = 0;
    SHQ_TRY(metal_emit_device(ctx, w, kernel_type, BoxSize, d_queue, nq, &np));
    if(npairs_out)
        *npairs_out = (int64_t) np;
    SHQ_HIP(hipMemsetAsync(d_massreturn, 0, sizeof(double) * (size_t) nq, st));
    if(np == 0)
        return SHQ_OK;
    SHQ_TRY(prim_sort_pairs(ctx, ctx->metal_keys[0].ptr, ctx->metal_keys[1].ptr, ctx->metal_val[0].ptr, ctx->metal_val[1].ptr, (size_t) np, 0, 64));
    /* thismass per pair, in (particle, star) order, into metal_val[0] */
    metal_apply_kernel<<<dim3(nblk((long long) np)), dim3(256), 0, st>>>((long long) np, ctx->metal_keys[1].ptr, nullptr, ctx->metal_val[1].ptr, *w, ctx->metal_val[0].ptr);
    SHQ_HIP(hipGetLastError());
    metal_rekey_kernel<<<dim3(nblk((long long) np)), dim3(256), 0, st>>>((long long) np, ctx->metal_keys[1].ptr, ctx->metal_keys[0].ptr);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(prim_sort_pairs(ctx, ctx->metal_keys[0].ptr, ctx->metal_keys[1].ptr, ctx->metal_val[0].ptr, ctx->metal_val[1].ptr, (size_t) np, 0, 64));
    metal_sum_kernel<<<dim3(nblk((long long) np)), dim3(256), 0, st>>>((long long) np, ctx->metal_keys[1].ptr, ctx->metal_val[1].ptr, d_massreturn);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* ---- the same return in the parts a multi-rank driver needs (shenqi_amd/dist.py:DistMetalReturn) -------------------------------------
 * A triple that fell on an imported gas particle belongs to that particle's owner.  The route kernel rewrites every emitted entry (a
 * triple here, a record of the black-hole walks in sph_bh.hip) to (owner, row at the owner, position in the global queue); two stable
 * sorts, by (row, position) and then by owner, leave one order that the caller writes its list in and the driver cuts by the per-owner
 * counts.  The owner sorts what it gathered by (row, star) once more and applies it with metal_apply_kernel: the global queue order,
 * whatever rank a star lives on. */
#define METAL_ROUTE_LDS 1024 /* owners a workgroup counts in LDS before it adds to the global counts; more ranks count in global memory */
__global__ __launch_bounds__(256) void route_kernel(long long np, const unsigned long long *__restrict__ keys, long long nlocal, const int32_t *__restrict__ ghost_owner,
                                                    const int32_t *__restrict__ ghost_index, int nranks, int rank, unsigned long long queue_offset,
                                                    const int32_t *__restrict__ qpos, unsigned long long *__restrict__ routed, uint32_t *__restrict__ owner_out,
                                                    unsigned long long *counts)
{
    __shared__ unsigned int hist[METAL_ROUTE_LDS];
    const bool lds = nranks <= METAL_ROUTE_LDS;
    if(lds)
        for(int i = threadIdx.x; i < nranks; i += blockDim.x)
            hist[i] = 0;
    __syncthreads();
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k < np) {
        const long long p = (long long) (keys[k] >> 32);
        const unsigned long long t = keys[k] & 0xffffffffull;
        const bool own = p < nlocal;
        const unsigned o = (unsigned) (own ? rank : ghost_owner[p - nlocal]);
        const unsigned idx = (unsigned) (own ? (int32_t) p : ghost_index[p - nlocal]);
        routed[k] = ((unsigned long long) idx << 32) | (queue_offset + (qpos ? (unsigned long long) qpos[t] : t));
        owner_out[k] = o;
        if(lds)
            atomicAdd(&hist[o], 1u);
        else
            atomicAdd(&counts[o], 1ull);
    }
    __syncthreads();
    if(lds)
        for(int i = threadIdx.x; i < nranks; i += blockDim.x)
            if(hist[i])
                atomicAdd(&counts[i], (unsigned long long) hist[i]);
}

__global__ void gather_u32_kernel(long long n, const uint32_t *__restrict__ src, const uint32_t *__restrict__ ord, uint32_t *out)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k < n)
        out[k] = src[ord[k]];
}

int shq_route_sort(shq_context *ctx, int64_t n, int64_t nlocal, const int32_t *d_ghost_owner, const int32_t *d_ghost_index, int nranks, int rank, int64_t queue_offset,
                   const int32_t *d_qpos, unsigned long long *d_counts)
{
    hipStream_t st = ctx->stream;
    uint32_t *owner = ctx->metal_u32[0].ptr, *ord1 = ctx->metal_u32[1].ptr, *okey = ctx->metal_u32[2].ptr, *ord2 = ctx->metal_u32[3].ptr;
    unsigned long long *routed = ctx->metal_keys[1].ptr;
    route_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, ctx->metal_keys[0].ptr, nlocal, d_ghost_owner, d_ghost_index, nranks, rank, (unsigned long long) queue_offset, d_qpos,
                                                      routed, owner, d_counts);
    SHQ_HIP(hipGetLastError());
    /* by (row at the owner, position); the sorted keys themselves are not needed (they land on the emitted keys, which are done with) */
    SHQ_TRY(prim_sort_pairs(ctx, routed, ctx->metal_keys[0].ptr, rocprim::counting_iterator<uint32_t>(0), ord1, (size_t) n, 0, 64));
    /* then, stable, by owner */
    gather_u32_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, owner, ord1, okey);
    SHQ_HIP(hipGetLastError());
    unsigned bits = 1;
    while(bits < 32 && (1ull << bits) < (unsigned long long) nranks)
        bits++;
    return prim_sort_pairs(ctx, okey, owner, ord1, ord2, (size_t) n, 0, bits); /* `owner` is free again: every entry went into okey */
}

__global__ void metal_trip_write_kernel(long long n, const uint32_t *__restrict__ owner_sorted, const uint32_t *__restrict__ ord, const unsigned long long *__restrict__ routed,
                                        const double *__restrict__ wk, shq_metal_triple *out)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    const size_t j = ord[k];
    shq_metal_triple T;
    T.owner = (int32_t) owner_sorted[k];
    T.part_index = (int32_t) (routed[j] >> 32);
    T.star = (uint32_t) (routed[j] & 0xffffffffull);
    T.pad_ = 0;
    T.wk = wk[j];
    out[k] = T;
}

int shq_metal_triples_device(shq_context *ctx, MetalWalkArgs *w, int kernel_type, double BoxSize, const int32_t *d_queue, int64_t nq, int64_t nlocal,
                             const int32_t *d_ghost_owner, const int32_t *d_ghost_index, int nranks, int rank, int64_t queue_offset,
                             unsigned long long *d_counts, int64_t *ntriples)
{
    hipStream_t st = ctx->stream;
    *ntriples = 0;
    SHQ_HIP(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * (size_t) nranks, st));
    if(nq == 0)
        return SHQ_OK;
    unsigned long long np = 0;
    SHQ_TRY(metal_emit_device(ctx, w, kernel_type, BoxSize, d_queue, nq, &np));
    if(np == 0)
        return SHQ_OK;
    SHQ_CHECK(np < (1ull << 32), SHQ_ERR_INVALID, "metal_return_triples: %llu triples, the sort orders are 32 bits", np);
    for(auto &b : ctx->metal_u32)
        SHQ_TRY(b.reserve((size_t) np));
    SHQ_TRY(ctx->metal_trip.reserve((size_t) np * sizeof(shq_metal_triple)));
    const long long n = (long long) np;
    SHQ_TRY(shq_route_sort(ctx, n, nlocal, d_ghost_owner, d_ghost_index, nranks, rank, queue_offset, nullptr, d_counts));
    metal_trip_write_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, ctx->metal_u32[0].ptr, ctx->metal_u32[3].ptr, ctx->metal_keys[1].ptr, ctx->metal_val[0].ptr,
                                                                 reinterpret_cast<shq_metal_triple *>(ctx->metal_trip.ptr));
    SHQ_HIP(hipGetLastError());
    *ntriples = (int64_t) np;
    return SHQ_OK;
}

__global__ void metal_trip_keys_kernel(long long n, const shq_metal_triple *__restrict__ trip, unsigned long long *keys, double *wk)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    keys[k] = ((unsigned long long) (uint32_t) trip[k].part_index << 32) | (unsigned long long) trip[k].star;
    wk[k] = trip[k].wk;
}

int shq_metal_apply_device(shq_context *ctx, const MetalWalkArgs *w, const shq_metal_triple *d_trip, int64_t n, double *d_thismass)
{
    if(n == 0)
        return SHQ_OK;
    hipStream_t st = ctx->stream;
    SHQ_CHECK(n < (1ll << 32), SHQ_ERR_INVALID, "metal_return_apply: %lld triples, the sort orders are 32 bits", (long long) n);
    SHQ_TRY(ctx->metal_keys[0].reserve((size_t) n));
    SHQ_TRY(ctx->metal_keys[1].reserve((size_t) n));
    SHQ_TRY(ctx->metal_val[0].reserve((size_t) n));
    SHQ_TRY(ctx->metal_u32[0].reserve((size_t) n));
    metal_trip_keys_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, d_trip, ctx->metal_keys[0].ptr, ctx->metal_val[0].ptr);
    SHQ_HIP(hipGetLastError());
    /* the carried original index is the sort's value column */
    SHQ_TRY(prim_sort_pairs(ctx, ctx->metal_keys[0].ptr, ctx->metal_keys[1].ptr, rocprim::counting_iterator<uint32_t>(0), ctx->metal_u32[0].ptr, (size_t) n, 0, 64));
    metal_apply_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, ctx->metal_keys[1].ptr, ctx->metal_u32[0].ptr, ctx->metal_val[0].ptr, *w, d_thismass);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

__global__ void metal_sums_key1_kernel(long long n, const int32_t *__restrict__ owner, const int32_t *__restrict__ pidx, unsigned long long *keys)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k < n)
        keys[k] = ((unsigned long long) (uint32_t) owner[k] << 32) | (unsigned long long) (uint32_t) pidx[k];
}

/* the star's key in the upper half, as metal_sum_kernel reads it; the lower half is zero */
__global__ void metal_sums_key2_kernel(long long n, const int32_t *__restrict__ qpos, const double *__restrict__ thismass, const uint32_t *__restrict__ ord,
                                       unsigned long long *keys, double *val)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    const size_t j = ord[k];
    keys[k] = (unsigned long long) (uint32_t) qpos[j] << 32;
    val[k] = thismass[j];
}

int shq_metal_sums_device(shq_context *ctx, const int32_t *d_qpos, const int32_t *d_owner, const int32_t *d_pidx, const double *d_thismass, int64_t n, int64_t nq,
                          double *d_massreturn)
{
    hipStream_t st = ctx->stream;
    if(nq > 0)
        SHQ_HIP(hipMemsetAsync(d_massreturn, 0, sizeof(double) * (size_t) nq, st));
    if(n == 0 || nq == 0)
        return SHQ_OK;
    SHQ_CHECK(n < (1ll << 32), SHQ_ERR_INVALID, "metal_return_sums: %lld triples, the sort orders are 32 bits", (long long) n);
    for(int i = 0; i < 2; i++) {
        SHQ_TRY(ctx->metal_keys[i].reserve((size_t) n));
        SHQ_TRY(ctx->metal_val[i].reserve((size_t) n));
    }
    SHQ_TRY(ctx->metal_u32[0].reserve((size_t) n));
    /* by (owner, particle) first, then, stable, by the star: the existing rekey, sort and sum with a wider key */
    metal_sums_key1_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, d_owner, d_pidx, ctx->metal_keys[0].ptr);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(prim_sort_pairs(ctx, ctx->metal_keys[0].ptr, ctx->metal_keys[1].ptr, rocprim::counting_iterator<uint32_t>(0), ctx->metal_u32[0].ptr, (size_t) n, 0, 64));
    metal_sums_key2_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, d_qpos, d_thismass, ctx->metal_u32[0].ptr, ctx->metal_keys[0].ptr, ctx->metal_val[0].ptr);
    SHQ_HIP(hipGetLastError());
    /* all 64 bits, the lower half being zero: a bit range that ends at bit 64 and does not start at 0 is beyond what the sort's small-size path compares */
    SHQ_TRY(prim_sort_pairs(ctx, ctx->metal_keys[0].ptr, ctx->metal_keys[1].ptr, ctx->metal_val[0].ptr, ctx->metal_val[1].ptr, (size_t) n, 0, 64));
    metal_sum_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, ctx->metal_keys[1].ptr, ctx->metal_val[1].ptr, d_massreturn);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* ---- the wind model's particle loops: winds_evolve (winds.cpp:370-387) and winds_subgrid / winds_make_after_sf (:272-292, 567-585) -- */
__global__ void winds_evolve_kernel(long long n, const int32_t *list, const uint8_t *pflags, const uint8_t *bin_hydro, const double *density, double *delay,
                                    double a3inv, double hubble, double DensThresh, double MaxTravelTime, shq_kick_factors kf)
{
#pragma clang fp contract(off)
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= n)
        return;
    const long long i = list ? (long long) list[t] : t;
    const unsigned f = pflags[i];
    if((f >> 4) != 0 || (f & 1u))
        return;
    double d = delay[i];
    if(d > 0 && density[i] * a3inv < DensThresh)
        d = 0;
    if(d > 0) {
        if(d > MaxTravelTime)
            d = MaxTravelTime;
        const double dtime = kf.dloga_for_bin[bin_hydro[i]] / hubble;
        d = fmax(d - dtime, 0);
    }
    delay[i] = d;
}

__global__ void winds_subgrid_kernel(long long n, const int32_t *list, const double *stellarmass, const double *vdisp, const double4 *posm, const WindWalkArgs w, double *vel,
                                     double *entropy, const double *density, double *delay, unsigned long long *nkicked)
{
#pragma clang fp contract(off)
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= n)
        return;
    const long long i = list ? (long long) list[t] : t;
    /* get_wind_params, :489-507 */
    const double time = w.P.Time;
    const double vphys = vdisp[t] / time;
    const double utherm = w.P.WindThermalFactor * 1.5 * vphys * vphys;
    double windeff, v;
    if(w.P.WindModel & 8) {
        windeff = w.P.WindEfficiency;
        v = w.P.WindSpeed * time;
    } else {
        windeff = (w.P.WindSigma0 * w.P.WindSigma0) / (vphys * vphys + 2 * utherm);
        v = w.P.WindSpeedFactor * vdisp[t];
    }
    if(v < w.P.MinWindVelocity * time)
        v = w.P.MinWindVelocity * time;
    /* winds_make_after_sf: the Springel & Hernquist 03 probability */
    const double pw = windeff * stellarmass[t] / posm[i].w;
    const double prob = 1 - exp(-pw);
    const unsigned long long id = w.ids[i];
    if(!(w.rnd[(id + 2) % w.rndsize] < prob))
        return;
    if(v > 0 && time > 0) { /* wind_do_kick */
        const double theta = acos(2 * w.rnd[(id + 3) % w.rndsize] - 1);
        const double phi = 2 * M_PI * w.rnd[(id + 4) % w.rndsize];
        const double dir[3] = {sin(theta) * cos(phi), sin(theta) * sin(phi), cos(theta)};
        for(int j = 0; j < 3; j++)
            vel[3 * i + j] += v * dir[j];
        const double enttou = pow(density[i] / pow(time, 3), SPH_GAMMA_MINUS1) / SPH_GAMMA_MINUS1;
        entropy[i] += utherm / enttou;
        if((w.P.WindModel & 2) && w.P.MaxWindFreeTravelTime > 0) {
            double d = w.P.WindFreeTravelLength / (v / time);
            if(d > w.P.MaxWindFreeTravelTime)
                d = w.P.MaxWindFreeTravelTime;
            delay[i] = d;
        }
        atomicAdd(nkicked, 1ull);
    }
}

int shq_winds_evolve_device(shq_context *ctx, const int32_t *d_list, int64_t n, double a3inv, double hubble, double DensThresh, double MaxTravelTime,
                            const shq_kick_factors *kf)
{
    if(n > 0)
        winds_evolve_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(n, d_list, ctx->pflags.ptr, ctx->bin_hydro.ptr, ctx->g_density.ptr, ctx->g_delaytime.ptr, a3inv,
                                                                         hubble, DensThresh, MaxTravelTime, *kf);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

int shq_winds_subgrid_device(shq_context *ctx, const WindWalkArgs *w, const int32_t *d_list, int64_t n, const double *d_stellarmass, const double *d_vdisp,
                             unsigned long long *d_nkicked)
{
    if(n > 0)
        winds_subgrid_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(n, d_list, d_stellarmass, d_vdisp, ctx->posm.ptr, *w, ctx->vel.ptr, ctx->g_entropy.ptr,
                                                                          ctx->g_density.ptr, ctx->g_delaytime.ptr, d_nkicked);
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}
