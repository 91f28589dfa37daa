/* lightcone.hip — light-cone crossings on device-resident records (include/shenqi_hip.h, "Light-cone crossings").
 *
 *   lightcone_get_horizon   lightcone.cpp:101-115            shq_lightcone_horizon    host
 *   lightcone_init          :95                              shq_lightcone_init       host
 *   lightcone_set_time      :118-200 (update_replicas)       shq_lightcone_set_time   host
 *   lightcone_compute       :159-168 over :203-250           shq_lightcone_compute    two kernels around a scan
 *
 * The kernels.  One lane per particle; the replica loop runs in lockstep across the wave, so the replica shift is the same for all 64
 * lanes and is read from a const array by a uniform index (scalar loads): three doubles per trip are all the scalar work of the loop body.
 * A lane keeps Pos, its drift Vel * ddrift, ID and a count.  The distance test comes first: the draw of (p, i) is gathered from the random
 * table only in trips where some lane of the wave passes it (a scalar branch on the ballot), which is rare - a step sweeps a thin shell.
 * Pass A stores the crossings of every particle and the replicas of its first two, an exclusive scan turns the counts into row
 * offsets, and pass B writes every particle's rows at its own offset: rows come out ordered by (particle, replica) whatever the
 * scheduling, and no atomic decides a position.  In pass B a lane with one or two rows (nearly all that have any) computes just the pairs
 * pass A noted; only lanes with more run the loop again.  A workgroup of pass B whose offsets do not move leaves on two scalar loads.
 * Both passes compute a pair by the same functions, so that they cannot disagree. */
#include "device_prims.hpp"
#include "call_scope.hpp"
#include <math.h>
#include <string.h>

namespace {

constexpr int LC_BLOCK = 256;
constexpr size_t LC_MAXREC = 480; /* the bound of shq_io_gather */

struct LcArgs {
    const char *parts;
    unsigned elsize, off_type, off_pos, off_vel, off_id;
    long long numpart;
    const double *reps; /* [nrep][3] */
    int nrep;
    double H, H2, Hprev, H2prev, frac;
    double ddrift, off[3];
    const double *rnd;
    unsigned long long rndsize;
};

/* :219-223 for replica shift R: the two positions and their squared distances.  vd = Vel[k] * ddrift (MyFloat is double in these records), of particle p
 * (CONSISTENT) or of record i (AS_WRITTEN).  The sums start from the first square: 0 + x is x for a square, which is never -0. */
template <int MODE>
__device__ __forceinline__ void lc_ends(const double pos[3], const double vd[3], const double R[3], const double off[3], double pold[3], double pnew[3], double *dold,
                                        double *dnew)
{
#pragma clang fp contract(off)
#pragma unroll
    for(int k = 0; k < 3; k++) {
        const double shifted = pos[k] + R[k];
        pold[k] = shifted - off[k];
        pnew[k] = ((MODE == SHQ_LIGHTCONE_CONSISTENT ? shifted : pos[k]) + vd[k]) - off[k];
    }
    *dnew = pnew[0] * pnew[0];
    *dnew += pnew[1] * pnew[1];
    *dnew += pnew[2] * pnew[2];
    *dold = pold[0] * pold[0];
    *dold += pold[1] * pold[1];
    *dold += pold[2] * pold[2];
}

/* :227-246: the interpolated crossing of one pair into row r */
__device__ __forceinline__ void lc_row(const LcArgs &a, const double pold[3], const double pnew[3], double dold, double dnew, long long r, long long p, int i,
                                       double *__restrict__ rows, int32_t *__restrict__ index, int32_t *__restrict__ replica)
{
#pragma clang fp contract(off)
    double u1, u2;
    if(dold != dnew) {
        dnew = sqrt(dnew);
        dold = sqrt(dold);
        const double cnew = dnew - a.H, cold = dold - a.Hprev;
        u1 = -cold / (cnew - cold);
        u2 = cnew / (cnew - cold);
    } else
        u1 = u2 = 0.5; /* "this particle is moving along the horizon" */
    double *o = rows + 4 * (size_t) r;
    o[0] = pold[0] * u2 + pnew[0] * u1;
    o[1] = pold[1] * u2 + pnew[1] * u1;
    o[2] = pold[2] * u2 + pnew[2] * u1;
    o[3] = a.frac;
    if(index)
        index[r] = (int32_t) p;
    if(replica)
        replica[r] = i;
}

/* Base[i].Vel * ddrift: record i, the replica index; the caller has seen numpart >= nrep */
__device__ __forceinline__ void lc_drift_of_record(const LcArgs &a, int i, double vd[3])
{
#pragma clang fp contract(off)
    const double *V = reinterpret_cast<const double *>(a.parts + (size_t) i * a.elsize + a.off_vel);
    vd[0] = V[0] * a.ddrift, vd[1] = V[1] * a.ddrift, vd[2] = V[2] * a.ddrift;
}

/* EMIT false (pass A): cnt[p] = the crossings of particle p, two[p] = the replicas of its first two (16 bits each).
 * EMIT true (pass B): the rows of particle p from row off[p] on.  A particle with one or two rows - nearly all that have any - finds its
 * replicas in two[p] and computes just those pairs; one with more runs the loop again, in lockstep with the other such lanes of its wave. */
template <int MODE, bool EMIT>
__global__ __launch_bounds__(LC_BLOCK) void lc_kernel(LcArgs a, int32_t *__restrict__ cnt, int32_t *__restrict__ two, const long long *__restrict__ off,
                                                      double *__restrict__ rows, int32_t *__restrict__ index, int32_t *__restrict__ replica)
{
#pragma clang fp contract(off)
    const long long p0 = (long long) blockIdx.x * LC_BLOCK;
    if(EMIT) { /* uniform: nothing of this workgroup crossed */
        const long long pend = p0 + LC_BLOCK < a.numpart ? p0 + LC_BLOCK : a.numpart;
        if(off[pend] == off[p0])
            return;
    }
    const long long p = p0 + threadIdx.x;
    bool live = p < a.numpart;
    long long row = 0, mine = 0;
    if(EMIT && live) {
        row = off[p];
        mine = off[p + 1] - row;
        live = mine != 0;
    }
    const char *rec = a.parts + (size_t) (live ? p : 0) * a.elsize;
    if(live && !EMIT)
        live = *reinterpret_cast<const uint8_t *>(rec + a.off_type) == 1; /* "DM only"; no garbage test */
    double pos[3] = {0, 0, 0}, vd[3] = {0, 0, 0};
    unsigned long long id = 0;
    if(live) {
        const double *P = reinterpret_cast<const double *>(rec + a.off_pos);
        pos[0] = P[0], pos[1] = P[1], pos[2] = P[2];
        id = *reinterpret_cast<const unsigned long long *>(rec + a.off_id);
        if(MODE == SHQ_LIGHTCONE_CONSISTENT) {
            const double *V = reinterpret_cast<const double *>(rec + a.off_vel);
            vd[0] = V[0] * a.ddrift, vd[1] = V[1] * a.ddrift, vd[2] = V[2] * a.ddrift;
        }
    }
    const double offs[3] = {a.off[0], a.off[1], a.off[2]};
    if(EMIT) {
        if(live && mine <= 2) { /* the pairs pass A noted: each lane its own replicas */
            const unsigned both = (unsigned) two[p];
            for(int j = 0; j < (int) mine; j++) {
                const int i = (int) ((both >> (16 * j)) & 0xffffu); /* < nrep: pass A wrote it */
                const double R[3] = {a.reps[3 * i], a.reps[3 * i + 1], a.reps[3 * i + 2]};
                if(MODE == SHQ_LIGHTCONE_AS_WRITTEN)
                    lc_drift_of_record(a, i, vd);
                double pold[3], pnew[3], dold, dnew;
                lc_ends<MODE>(pos, vd, R, offs, pold, pnew, &dold, &dnew);
                lc_row(a, pold, pnew, dold, dnew, row + j, p, i, rows, index, replica);
            }
        }
        live = live && mine > 2;
    }
    int n = 0;
    unsigned both = 0;
    if(shq_ballot(live) != 0ull) { /* a wave without a particle to test skips the loop */
        for(int i = 0; i < a.nrep; i++) {
            const double R[3] = {a.reps[3 * i], a.reps[3 * i + 1], a.reps[3 * i + 2]};
            if(MODE == SHQ_LIGHTCONE_AS_WRITTEN) /* the same record for every lane */
                lc_drift_of_record(a, i, vd);
            double pold[3], pnew[3], dold, dnew;
            lc_ends<MODE>(pos, vd, R, offs, pold, pnew, &dold, &dnew);
            bool hit = live && dold <= a.H2prev && dnew >= a.H2;
            if(shq_ballot(hit) == 0ull)
                continue;
            if(hit) {
                const double r = a.rnd[(id + (unsigned long long) (long long) i) % a.rndsize];
                hit = !(r > a.frac); /* "if(r > SampleFraction) continue" */
            }
            if(!hit)
                continue;
            if(EMIT) {
                if(n < mine) /* always: both passes evaluate one predicate on the same data */
                    lc_row(a, pold, pnew, dold, dnew, row + n, p, i, rows, index, replica);
            } else if(n < 2)
                both |= (unsigned) i << (16 * n);
            n++;
        }
    }
    if(!EMIT && p <= a.numpart) { /* entry numpart is the zero behind the last */
        cnt[p] = n;
        two[p] = (int32_t) both;
    }
}

template <bool EMIT>
void lc_launch(int mode, hipStream_t st, const LcArgs &a, int32_t *cnt, int32_t *two, const long long *off, double *rows, int32_t *index, int32_t *replica)
{
    const dim3 grid(nblk(a.numpart + (EMIT ? 0 : 1), LC_BLOCK)), block(LC_BLOCK);
    if(mode == SHQ_LIGHTCONE_CONSISTENT)
        lc_kernel<SHQ_LIGHTCONE_CONSISTENT, EMIT><<<grid, block, 0, st>>>(a, cnt, two, off, rows, index, replica);
    else
        lc_kernel<SHQ_LIGHTCONE_AS_WRITTEN, EMIT><<<grid, block, 0, st>>>(a, cnt, two, off, rows, index, replica);
}

int lc_check_table(const shq_lightcone_table *t)
{
    SHQ_CHECK(t && t->tab_loga && t->tab_Dc, SHQ_ERR_INVALID, "lightcone: null table");
    SHQ_CHECK(t->nentry >= 2 && t->dloga > 0 && std::isfinite(t->dloga), SHQ_ERR_INVALID, "lightcone: a table has at least 2 entries and dloga > 0");
    return SHQ_OK;
}

/* :101-115 */
double lc_horizon(const shq_lightcone_table *t, const double a)
{
#pragma clang fp contract(off)
    const double *tab_loga = t->tab_loga, *tab_Dc = t->tab_Dc;
    const int NENTRY = t->nentry;
    double loga = log(a);
    const double fbin = (log(a) - tab_loga[0]) / t->dloga;
    /* the reference converts to int whatever comes out; a value no int holds can only lie beyond one end of the table */
    if(!(fbin > -2147483648.0))
        return tab_Dc[0];
    if(!(fbin < 2147483647.0))
        return tab_Dc[NENTRY - 1];
    int bin = (int) fbin;
    if(bin < 0) {
        return tab_Dc[0];
    }
    if(bin >= NENTRY - 1) {
        return tab_Dc[NENTRY - 1];
    }
    double u1 = loga - tab_loga[bin];
    double u2 = tab_loga[bin + 1] - loga;
    u1 /= (tab_loga[bin + 1] - tab_loga[bin]);
    u2 /= (tab_loga[bin + 1] - tab_loga[bin]);
    return tab_Dc[bin] * u2 + tab_Dc[bin + 1] * u1;
}

int lc_check_params(const shq_lightcone_params *p)
{
    SHQ_CHECK(p, SHQ_ERR_INVALID, "lightcone: null parameters");
    SHQ_CHECK(p->BoxBoost >= 1 && p->BoxBoost <= 1290, SHQ_ERR_INVALID, "lightcone: BoxBoost = %d outside 1 .. 1290", p->BoxBoost);
    SHQ_CHECK(p->ReferenceRedshift > -1 && std::isfinite(p->ReferenceRedshift), SHQ_ERR_INVALID, "lightcone: ReferenceRedshift = %g", p->ReferenceRedshift);
    return SHQ_OK;
}

} // namespace

extern "C" int shq_lightcone_horizon(const shq_lightcone_table *t, double a, double *Dc)
{
    SHQ_TRY(lc_check_table(t));
    SHQ_CHECK(Dc, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(a > 0, SHQ_ERR_INVALID, "lightcone_horizon: a = %g", a);
    *Dc = lc_horizon(t, a);
    return SHQ_OK;
}

extern "C" int shq_lightcone_init(const shq_lightcone_table *t, const shq_lightcone_params *p, shq_lightcone_state *s)
{
#pragma clang fp contract(off)
    SHQ_TRY(lc_check_table(t));
    SHQ_TRY(lc_check_params(p));
    SHQ_CHECK(s, SHQ_ERR_INVALID, "null argument");
    memset(s, 0, sizeof(*s));
    s->HorizonDistanceRef = lc_horizon(t, 1 / (1 + p->ReferenceRedshift));
    return SHQ_OK;
}

extern "C" int shq_lightcone_set_time(const shq_lightcone_table *t, const shq_lightcone_params *p, double a, double BoxSize, shq_lightcone_state *s)
{
#pragma clang fp contract(off)
    SHQ_TRY(lc_check_table(t));
    SHQ_TRY(lc_check_params(p));
    SHQ_CHECK(s, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(a > 0 && std::isfinite(a) && std::isfinite(BoxSize), SHQ_ERR_INVALID, "lightcone_set_time: a = %g, BoxSize = %g", a, BoxSize);
    double z = 1 / a - 1;
    if(z > p->zmin && z < p->zmax) {
        s->HorizonDistancePrev = s->HorizonDistance;
        s->HorizonDistance2Prev = s->HorizonDistance2;
        s->HorizonDistance = lc_horizon(t, a);
        s->HorizonDistance2 = s->HorizonDistance * s->HorizonDistance;
        /* update_replicas */
        const int BoxBoost = p->BoxBoost;
        int Nmax = BoxBoost * BoxBoost * BoxBoost;
        int i;
        int rx, ry, rz;
        rx = ry = rz = 0;
        s->Nreplica = 0;
        for(i = 0; i < Nmax; i++) {
            double dx = BoxSize * rx;
            double dy = BoxSize * ry;
            double dz = BoxSize * rz;
            double d1, d2;
            d1 = dx * dx + dy * dy + dz * dz;
            dx += BoxSize;
            dy += BoxSize;
            dz += BoxSize;
            d2 = dx * dx + dy * dy + dz * dz;
            if(d1 <= s->HorizonDistance2 && d2 >= s->HorizonDistance2) {
                /* the reference writes entry 1000 of its 8192 before it ends the run; this array ends at 1000 */
                SHQ_CHECK(s->Nreplica < SHQ_LIGHTCONE_MAXREPLICA, SHQ_ERR_INVALID, "too many replica");
                s->Reps[s->Nreplica][0] = rx * BoxSize;
                s->Reps[s->Nreplica][1] = ry * BoxSize;
                s->Reps[s->Nreplica][2] = rz * BoxSize;
                s->Nreplica++;
            }
            rz++;
            if(rz == BoxBoost) {
                rz = 0;
                ry++;
            }
            if(ry == BoxBoost) {
                ry = 0;
                rx++;
            }
        }
        if(z < p->ReferenceRedshift) {
            s->SampleFraction = 1.0;
        } else {
            /* "This is the angular resolution rule" */
            s->SampleFraction = s->HorizonDistanceRef / s->HorizonDistance;
            s->SampleFraction *= s->SampleFraction;
            s->SampleFraction *= s->SampleFraction;
        }
    } else {
        s->SampleFraction = 0;
    }
    return SHQ_OK;
}

extern "C" int shq_lightcone_compute(shq_context *ctx, const shq_lightcone_layout *layout, const void *d_parts, int64_t numpart, const shq_lightcone_state *s, int mode,
                                     double ddrift, const double CurrentParticleOffset[3], const double *rnd_table, int64_t rnd_size, double *d_rows, int32_t *d_index,
                                     int32_t *d_replica, int64_t capacity, int64_t *nrows)
{
    SHQ_CHECK(ctx && layout && s && CurrentParticleOffset && rnd_table && nrows, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(mode == SHQ_LIGHTCONE_CONSISTENT || mode == SHQ_LIGHTCONE_AS_WRITTEN, SHQ_ERR_INVALID, "lightcone_compute: mode %d", mode);
    SHQ_CHECK(numpart >= 0 && numpart < (1ll << 31) - 200 && (d_parts || numpart == 0), SHQ_ERR_INVALID, "lightcone_compute: bad particle array");
    const size_t es = layout->part_elsize;
    SHQ_CHECK(es >= 8 && es % 8 == 0 && es <= LC_MAXREC && ((uintptr_t) d_parts % 8) == 0, SHQ_ERR_INVALID,
              "lightcone_compute: records are 8-byte aligned, a multiple of 8 and at most %zu bytes", LC_MAXREC);
    SHQ_CHECK(layout->off_type < es && layout->off_pos % 8 == 0 && layout->off_pos + 24 <= es && layout->off_vel % 8 == 0 && layout->off_vel + 24 <= es &&
                  layout->off_id % 8 == 0 && layout->off_id + 8 <= es,
              SHQ_ERR_INVALID, "lightcone_compute: Type, Pos, Vel and ID must lie inside the record, aligned");
    SHQ_CHECK(rnd_size > 0, SHQ_ERR_INVALID, "lightcone_compute: empty random table");
    SHQ_CHECK(capacity >= 0 && (d_rows || capacity == 0), SHQ_ERR_INVALID, "lightcone_compute: no room for the rows");
    SHQ_CHECK(((uintptr_t) d_rows % 8) == 0 && ((uintptr_t) d_index % 4) == 0 && ((uintptr_t) d_replica % 4) == 0, SHQ_ERR_INVALID, "lightcone_compute: misaligned output");
    SHQ_CHECK(std::isfinite(ddrift) && std::isfinite(CurrentParticleOffset[0]) && std::isfinite(CurrentParticleOffset[1]) && std::isfinite(CurrentParticleOffset[2]),
              SHQ_ERR_INVALID, "lightcone_compute: ddrift and the offsets must be finite");
    SHQ_CHECK(std::isfinite(s->HorizonDistance) && std::isfinite(s->HorizonDistance2) && std::isfinite(s->HorizonDistancePrev) && std::isfinite(s->HorizonDistance2Prev) &&
                  std::isfinite(s->SampleFraction),
              SHQ_ERR_INVALID, "lightcone_compute: a horizon or SampleFraction is not finite");
    SHQ_CHECK(s->Nreplica >= 0 && s->Nreplica <= SHQ_LIGHTCONE_MAXREPLICA, SHQ_ERR_INVALID, "lightcone_compute: Nreplica = %d", s->Nreplica);
    SHQ_CHECK(mode != SHQ_LIGHTCONE_AS_WRITTEN || numpart >= s->Nreplica, SHQ_ERR_INVALID,
              "lightcone_compute: as written, replica i reads the velocity of record i: %ld records for %d replicas", (long) numpart, s->Nreplica);
    *nrows = 0;
    if(s->SampleFraction <= 0.0 || s->Nreplica == 0 || numpart == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(shq_join_pm(ctx));
    SHQ_TRY(shq_walk_check_status(ctx, false));
    hipStream_t st = ctx->stream;
    const size_t N = (size_t) numpart, nrep = (size_t) s->Nreplica;
    SHQ_TRY(ctx->lc_reps.reserve(3 * nrep));
    SHQ_TRY(ctx->lc_cnt.reserve(2 * (N + 1))); /* counts, then the first two replicas of every particle */
    SHQ_TRY(ctx->lc_off.reserve(N + 1));
    SHQ_TRY(ctx->bhw_rnd.reserve((size_t) rnd_size));
    SHQ_HIP(hipMemcpyAsync(ctx->lc_reps.ptr, &s->Reps[0][0], sizeof(double) * 3 * nrep, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(ctx->bhw_rnd.ptr, rnd_table, sizeof(double) * (size_t) rnd_size, hipMemcpyHostToDevice, st));
    LcArgs a;
    memset(&a, 0, sizeof(a));
    a.parts = (const char *) d_parts;
    a.elsize = (unsigned) es, a.off_type = (unsigned) layout->off_type, a.off_pos = (unsigned) layout->off_pos;
    a.off_vel = (unsigned) layout->off_vel, a.off_id = (unsigned) layout->off_id;
    a.numpart = (long long) numpart;
    a.reps = ctx->lc_reps.ptr;
    a.nrep = s->Nreplica;
    a.H = s->HorizonDistance, a.H2 = s->HorizonDistance2, a.Hprev = s->HorizonDistancePrev, a.H2prev = s->HorizonDistance2Prev, a.frac = s->SampleFraction;
    a.ddrift = ddrift;
    for(int k = 0; k < 3; k++)
        a.off[k] = CurrentParticleOffset[k];
    a.rnd = ctx->bhw_rnd.ptr;
    a.rndsize = (unsigned long long) rnd_size;

    CallScope sc(ctx, "lightcone_compute"); /* the events of the phase times */
    SHQ_TRY(sc.mark(st));
    lc_launch<false>(mode, st, a, ctx->lc_cnt.ptr, ctx->lc_cnt.ptr + N + 1, nullptr, nullptr, nullptr, nullptr);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(sc.mark(st));
    SHQ_TRY(prim_exclusive_scan(ctx, ctx->lc_cnt.ptr, ctx->lc_off.ptr, 0ll, N + 1));
    SHQ_TRY(sc.mark(st));
    long long total = 0;
    SHQ_HIP(hipMemcpyAsync(&total, ctx->lc_off.ptr + N, sizeof(total), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    ctx->lc_ms[0] = sc.ms(0, 1);
    ctx->lc_ms[1] = sc.ms(1, 2);
    ctx->lc_ms[2] = 0;
    *nrows = (int64_t) total;
    SHQ_CHECK(total <= capacity, SHQ_ERR_NOMEM, "lightcone_compute: %lld crossings for a capacity of %ld rows", total, (long) capacity);
    if(total == 0)
        return SHQ_OK;
    SHQ_TRY(sc.mark(st));
    lc_launch<true>(mode, st, a, nullptr, ctx->lc_cnt.ptr + N + 1, ctx->lc_off.ptr, d_rows, d_index, d_replica);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(sc.mark(st));
    SHQ_HIP(hipStreamSynchronize(st));
    ctx->lc_ms[2] = sc.ms(3, 4);
    return SHQ_OK;
}

extern "C" int shq_lightcone_phase_ms(shq_context *ctx, double ms[3])
{
    SHQ_CHECK(ctx && ms, SHQ_ERR_INVALID, "null argument");
    for(int i = 0; i < 3; i++)
        ms[i] = ctx->lc_ms[i];
    return SHQ_OK;
}
