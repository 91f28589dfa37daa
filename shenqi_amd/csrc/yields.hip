/* yields.hip — stellar yields on the device: metal_return_init and the yields of metal_return_copy (libgadget/metal_return.cpp:157-462,
 * 539-569; include/shenqi_hip.h, "stellar yields").  One star per lane; the yield and lifetime tables (about 11 KB with
 * the reference's) are staged in LDS once per workgroup, the cosmic-time table (tens of KB) is read from global memory, two cells per
 * star.  The arithmetic is yields_math.hpp, shared with the host. */
#include "common.hpp"
#include <string.h>
#include <algorithm>

namespace {

template <typename T> inline const T *pfield(const shq_part_view *v, int64_t i, size_t off)
{
    return reinterpret_cast<const T *>(static_cast<const char *>(v->base) + (size_t) i * v->elsize + off);
}
template <typename T> inline T *sfield(const shq_star_yield_view *v, int64_t slot, size_t off)
{
    return reinterpret_cast<T *>(static_cast<char *>(v->base) + (size_t) slot * v->elsize + off);
}

enum { YIN_MASS = 0, YIN_FORMATION, YIN_LASTENRICH, YIN_TMR, YIN_METALLICITY, YIN_NCOL };
enum { YOUT_AGE = 0, YOUT_LOW, YOUT_HIGH, YOUT_MASSRETURN, YOUT_LASTENRICH, YOUT_NCOL };
enum { YFLAG_CLAMPED = 1, YFLAG_REWRITTEN = 2 };

struct TimeTab {
    const double *T, *dT;
    long long n;
    double loga0, dloga;
};

__device__ inline void stage_tables(const YieldDesc &d, const double *__restrict__ tab, double *sT)
{
    for(int i = threadIdx.x; i < d.ndoubles; i += blockDim.x)
        sT[i] = tab[i];
    __syncthreads();
}

/* metal_return_init's loop body (:431-460) for the entry k of the active list; arrays by list position, column-major with stride n */
__global__ __launch_bounds__(256) void yields_init_kernel(long long n, YieldDesc d, const double *__restrict__ tab, TimeTab tt, double atime,
                                                          const int32_t *__restrict__ slot, const double *__restrict__ in, double *__restrict__ out,
                                                          uint8_t *__restrict__ mark, uint8_t *__restrict__ flags)
{
    extern __shared__ double sT[];
    stage_tables(d, tab, sT);
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= n)
        return;
    if(slot[k] < 0) { /* not a star */
        mark[k] = 0;
        flags[k] = 0;
        return;
    }
    const double mass = in[YIN_MASS * n + k], tmr = in[YIN_TMR * n + k], Z = in[YIN_METALLICITY * n + k];
    double last = in[YIN_LASTENRICH * n + k];
    const double age = yield_age(tt.T, tt.dT, tt.n, tt.loga0, tt.dloga, in[YIN_FORMATION * n + k], atime);
    const double initialmass = mass + tmr;
    double lo, hi;
    yield_mass_bin_limits(sT, d, &lo, &hi, last, age, Z);
    double mr = initialmass * yield_mass_yield(sT, d, last, age, Z, lo, hi);
    const double worklimit = 1e-3 * (mass + tmr); /* metals_haswork (:129) */
    uint8_t fl = 0;
    /* guard against making a zero mass particle (:445-456) */
    if(tmr + mr > initialmass * d.maxmassfrac) {
        fl |= YFLAG_CLAMPED;
        mr = initialmass * d.maxmassfrac - tmr;
        if(mr < 0)
            mr = 0;
        if(mr < worklimit) {
            last = (double) (float) age;
            fl |= YFLAG_REWRITTEN;
        }
    }
    out[YOUT_AGE * n + k] = age;
    out[YOUT_LOW * n + k] = lo;
    out[YOUT_HIGH * n + k] = hi;
    out[YOUT_MASSRETURN * n + k] = mr;
    out[YOUT_LASTENRICH * n + k] = last;
    mark[k] = mr < worklimit ? 0 : 1;
    flags[k] = fl;
}

/* metal_return_copy's yields (:547-568) for queue position q = list position qpos[q]; qout: MassGenerated[nq], MetalGenerated[nq],
 * MetalSpeciesGenerated[nq][NMETALS] */
__global__ __launch_bounds__(256) void yields_queue_kernel(long long nq, long long n, YieldDesc d, const double *__restrict__ tab,
                                                           const int32_t *__restrict__ qpos, const double *__restrict__ in, const double *__restrict__ out,
                                                           double *__restrict__ qout)
{
    extern __shared__ double sT[];
    stage_tables(d, tab, sT);
    const long long q = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nq)
        return;
    const long long k = qpos[q];
    const double initialmass = in[YIN_MASS * n + k] + in[YIN_TMR * n + k];
    double y[1 + SHQ_YIELD_NMETALS];
    yield_metal_yield(sT, d, out[YOUT_LASTENRICH * n + k], out[YOUT_AGE * n + k], in[YIN_METALLICITY * n + k], out[YOUT_LOW * n + k], out[YOUT_HIGH * n + k], y);
    qout[q] = out[YOUT_MASSRETURN * n + k];
    /* "It should be positive! If it is not, this is some integration error in the yield table" (:558-561) */
    const double mg = initialmass * y[0];
    qout[nq + q] = mg < 0 ? 0 : mg;
    for(int i = 0; i < SHQ_YIELD_NMETALS; i++) {
        const double s = y[1 + i] * initialmass;
        qout[2 * nq + q * SHQ_YIELD_NMETALS + i] = s < 0 ? 0 : s;
    }
}

/* metal_return_postprocess (:581-589); rows: mass, TotalMassReturned, MassReturn, age -> new mass (float), new TotalMassReturned, LastEnrichmentMyr (float) */
__global__ void yields_postprocess_kernel(long long nq, const int32_t *__restrict__ queue, double *rows, double4 *posm)
{
    const long long q = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(q >= nq)
        return;
    const double mr = rows[2 * nq + q];
    const float m = (float) (rows[q] - mr);
    rows[q] = (double) m;
    rows[nq + q] += mr;
    rows[3 * nq + q] = (double) (float) rows[3 * nq + q];
    if(posm)
        posm[queue[q]].w = (double) m;
}

bool increasing(const double *a, int n)
{
    for(int i = 1; i < n; i++)
        if(!(a[i] > a[i - 1]))
            return false;
    return true;
}

} // namespace

extern "C" int shq_yields_init(shq_context *ctx, const shq_yield_tables *t, const shq_cosmic_time_table *times, const shq_yield_params *p, double *maxmassfrac)
{
    SHQ_CHECK(ctx && t && times && p, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(t->nmetals == SHQ_YIELD_NMETALS, SHQ_ERR_INVALID, "yields_init: nmetals = %d, the library was built for %d", t->nmetals, SHQ_YIELD_NMETALS);
    SHQ_CHECK(t->life_nmet >= 2 && t->life_nmass >= 2 && t->agb_nmet >= 2 && t->agb_nmass >= 2 && t->snii_nmet >= 2 && t->snii_nmass >= 2, SHQ_ERR_INVALID,
              "yields_init: every table axis needs at least two nodes");
    SHQ_CHECK(t->lifetime_metallicity && t->lifetime_masses && t->lifetime && t->agb_metallicities && t->agb_masses && t->agb_total_mass && t->agb_total_metals &&
                  t->agb_yield && t->snii_metallicities && t->snii_masses && t->snii_total_mass && t->snii_total_metals && t->snii_yield && t->sn1a_yields,
              SHQ_ERR_INVALID, "yields_init: a table pointer is NULL");
    SHQ_CHECK(increasing(t->lifetime_metallicity, t->life_nmet) && increasing(t->lifetime_masses, t->life_nmass) && increasing(t->agb_metallicities, t->agb_nmet) &&
                  increasing(t->agb_masses, t->agb_nmass) && increasing(t->snii_metallicities, t->snii_nmet) && increasing(t->snii_masses, t->snii_nmass),
              SHQ_ERR_INVALID, "yields_init: a table axis is not strictly increasing");
    SHQ_CHECK(t->agb_masses[0] >= 1, SHQ_ERR_INVALID, "yields_init: agb_masses[0] = %g < 1: the closed forms integrate the power-law branch of the IMF only", t->agb_masses[0]);
    SHQ_CHECK(t->agb_masses[0] <= p->SNAGBSWITCH && p->SNAGBSWITCH <= p->MAXMASS && p->imf_norm > 0 && p->HubbleParam > 0, SHQ_ERR_INVALID,
              "yields_init: needs agb_masses[0] <= SNAGBSWITCH <= MAXMASS, imf_norm > 0, HubbleParam > 0");
    SHQ_CHECK(t->lifetime_masses[0] <= t->agb_masses[0] && t->lifetime_masses[t->life_nmass - 1] >= p->MAXMASS, SHQ_ERR_INVALID,
              "yields_init: the lifetime table does not span [agb_masses[0], MAXMASS]");
    /* the root of do_rootfinding is taken as the inverse of one segment: the lifetimes must decrease with mass up to MAXMASS */
    for(int j = 1; j < t->life_nmass && t->lifetime_masses[j - 1] < p->MAXMASS; j++)
        for(int i = 0; i < t->life_nmet; i++)
            SHQ_CHECK(t->lifetime[j * t->life_nmet + i] < t->lifetime[(j - 1) * t->life_nmet + i], SHQ_ERR_INVALID,
                      "yields_init: lifetime does not decrease with mass at node (%d, %d)", j, i);
    SHQ_CHECK(times->n >= 2 && times->n < (1ll << 28) && times->dloga > 0 && times->T && times->dTdloga, SHQ_ERR_INVALID,
              "yields_init: the cosmic-time table needs n >= 2 nodes, dloga > 0 and both arrays");
    SHQ_TRY(shq_walk_check_status(ctx, false));
    SHQ_HIP(hipSetDevice(ctx->device));

    YieldDesc d;
    memset(&d, 0, sizeof(d));
    d.life_nmet = t->life_nmet; d.life_nmass = t->life_nmass;
    d.agb_nmet = t->agb_nmet; d.agb_nmass = t->agb_nmass;
    d.snii_nmet = t->snii_nmet; d.snii_nmass = t->snii_nmass;
    std::vector<double> h;
    auto put = [&h](const double *a, size_t n) {
        const int o = (int) h.size();
        h.insert(h.end(), a, a + n);
        return o;
    };
    auto put_powers = [&h](const double *m, int n, bool p13) {
        const int o = (int) h.size();
        for(int j = 0; j < n; j++)
            h.push_back(p13 ? yield_p13(m[j]) : yield_p03(m[j]));
        return o;
    };
    const size_t nl = (size_t) t->life_nmet * t->life_nmass, na = (size_t) t->agb_nmet * t->agb_nmass, ns = (size_t) t->snii_nmet * t->snii_nmass;
    d.o_life_met = put(t->lifetime_metallicity, t->life_nmet);
    d.o_life_mass = put(t->lifetime_masses, t->life_nmass);
    d.o_life = put(t->lifetime, nl);
    d.o_agb_met = put(t->agb_metallicities, t->agb_nmet);
    d.o_agb_mass = put(t->agb_masses, t->agb_nmass);
    d.o_agb = put(t->agb_total_mass, na);
    put(t->agb_total_metals, na);
    put(t->agb_yield, na * SHQ_YIELD_NMETALS);
    d.o_agb_p13 = put_powers(t->agb_masses, t->agb_nmass, true);
    d.o_agb_p03 = put_powers(t->agb_masses, t->agb_nmass, false);
    d.o_snii_met = put(t->snii_metallicities, t->snii_nmet);
    d.o_snii_mass = put(t->snii_masses, t->snii_nmass);
    d.o_snii = put(t->snii_total_mass, ns);
    put(t->snii_total_metals, ns);
    put(t->snii_yield, ns * SHQ_YIELD_NMETALS);
    d.o_snii_p13 = put_powers(t->snii_masses, t->snii_nmass, true);
    d.o_snii_p03 = put_powers(t->snii_masses, t->snii_nmass, false);
    d.o_sn1a = put(&t->sn1a_total_metals, 1);
    put(t->sn1a_yields, SHQ_YIELD_NMETALS);
    d.ndoubles = (int) h.size();
    SHQ_CHECK(h.size() * sizeof(double) <= 48 * 1024, SHQ_ERR_INVALID, "yields_init: the tables (%zu bytes) do not fit the 48 KB of LDS the kernels stage them in",
              h.size() * sizeof(double));
    d.Sn1aN0 = p->Sn1aN0; d.HubbleParam = p->HubbleParam; d.imf_norm = p->imf_norm; d.MAXMASS = p->MAXMASS; d.SNAGBSWITCH = p->SNAGBSWITCH;
    const double hubbletime = 1 / (p->HubbleParam * SHQ_YIELD_HUBBLE * SHQ_YIELD_SEC_PER_MEGAYEAR);
    d.sn1a_scale = p->Sn1aN0 / (1 - pow(hubbletime / 40, 1 - 1.12));
    /* "Maximum possible mass return" (:425), with the routine the kernel runs */
    d.maxmassfrac = yield_mass_yield(h.data(), d, 0, hubbletime, t->snii_metallicities[t->snii_nmet - 1], t->agb_masses[0], p->MAXMASS);

    hipStream_t st = ctx->stream;
    ctx->yld_have = false;
    SHQ_TRY(ctx->yld_tab.reserve(h.size()));
    SHQ_TRY(ctx->yld_time.reserve(2 * (size_t) times->n));
    SHQ_HIP(hipStreamSynchronize(st)); /* a kernel of an earlier call may still read the old tables */
    SHQ_HIP(hipMemcpyAsync(ctx->yld_tab.ptr, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(ctx->yld_time.ptr, times->T, sizeof(double) * (size_t) times->n, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(ctx->yld_time.ptr + times->n, times->dTdloga, sizeof(double) * (size_t) times->n, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipStreamSynchronize(st));
    ctx->yld_host.swap(h);
    ctx->yld_desc = d;
    ctx->yld_time_n = times->n;
    ctx->yld_loga0 = times->loga0;
    ctx->yld_dloga = times->dloga;
    ctx->yld_amin = exp(times->loga0);
    ctx->yld_amax = exp(times->loga0 + times->dloga * (double) (times->n - 1));
    ctx->yld_have = true;
    if(maxmassfrac)
        *maxmassfrac = d.maxmassfrac;
    return SHQ_OK;
}

extern "C" int shq_metal_yields(shq_context *ctx, const shq_part_view *parts, const shq_star_yield_view *stars, const int32_t *active, int64_t nactive, double atime,
                                double *StellarAges, double *LowDyingMass, double *HighDyingMass, double *MassReturn, int32_t *queue, int64_t *nqueue,
                                double *MassGenerated, double *MetalGenerated, double *MetalSpeciesGenerated, int64_t *nbad)
{
    SHQ_CHECK(ctx && parts && stars && nqueue, SHQ_ERR_INVALID, "null argument");
    *nqueue = 0;
    if(nbad)
        *nbad = 0;
    SHQ_CHECK(ctx->yld_have, SHQ_ERR_STATE, "metal_yields: call shq_yields_init first");
    SHQ_CHECK(parts->off_mass != SHQ_NOFIELD && parts->off_type != SHQ_NOFIELD && parts->off_pi != SHQ_NOFIELD, SHQ_ERR_INVALID,
              "metal_yields: the particle view needs Mass, Type and PI");
    const int64_t n = parts->numpart, cnt = active ? nactive : n;
    SHQ_CHECK(n >= 0 && cnt >= 0 && (n == 0 || parts->base), SHQ_ERR_INVALID, "metal_yields: bad particle view or list length");
    SHQ_CHECK(cnt == 0 || (StellarAges && LowDyingMass && HighDyingMass && MassReturn && queue && MassGenerated && MetalGenerated && MetalSpeciesGenerated),
              SHQ_ERR_INVALID, "metal_yields: an output array is NULL");
    SHQ_CHECK(stars->numslots == 0 || stars->base, SHQ_ERR_INVALID, "metal_yields: the star slot view is NULL");
    SHQ_TRY(shq_walk_check_status(ctx, false));
    if(cnt == 0)
        return SHQ_OK;
    /* pack what the kernel reads of the list's stars; the input check of the time table rides along */
    const size_t N = (size_t) cnt;
    std::vector<double> hin(YIN_NCOL * N, 0.0);
    std::vector<int32_t> hslot(N, -1);
    int64_t nstar = 0, outside = 0;
    for(int64_t k = 0; k < cnt; k++) {
        const int64_t i = active ? active[k] : k;
        SHQ_CHECK(i >= 0 && i < n, SHQ_ERR_INVALID, "metal_yields: active[%ld] = %ld out of range", (long) k, (long) i);
        if(*pfield<uint8_t>(parts, i, parts->off_type) != 4)
            continue;
        const int32_t pi = *pfield<int32_t>(parts, i, parts->off_pi);
        SHQ_CHECK(pi >= 0 && pi < stars->numslots, SHQ_ERR_INVALID, "metal_yields: star %ld has PI %d outside the slot array", (long) i, pi);
        hslot[(size_t) k] = pi;
        const double ft = (double) *sfield<float>(stars, pi, stars->off_formationtime);
        hin[YIN_MASS * N + k] = (double) *pfield<float>(parts, i, parts->off_mass);
        hin[YIN_FORMATION * N + k] = ft;
        hin[YIN_LASTENRICH * N + k] = (double) *sfield<float>(stars, pi, stars->off_lastenrichmentmyr);
        hin[YIN_TMR * N + k] = *sfield<double>(stars, pi, stars->off_totalmassreturned);
        hin[YIN_METALLICITY * N + k] = *sfield<double>(stars, pi, stars->off_metallicity);
        nstar++;
        if(!(ft >= ctx->yld_amin && ft <= ctx->yld_amax))
            outside++;
    }
    if(nstar > 0 && !(atime >= ctx->yld_amin && atime <= ctx->yld_amax))
        outside = nstar;
    if(outside > 0) {
        if(nbad)
            *nbad = outside;
        SHQ_CHECK(false, SHQ_ERR_INVALID, "metal_yields: %ld star(s) with FormationTime, or atime = %g, outside the cosmic-time table [%g, %g]", (long) outside, atime,
                  ctx->yld_amin, ctx->yld_amax);
    }
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SHQ_TRY(ctx->yld_in.reserve(YIN_NCOL * N));
    SHQ_TRY(ctx->yld_out.reserve((YOUT_NCOL + 2 + SHQ_YIELD_NMETALS) * N));
    SHQ_TRY(ctx->yld_i32.reserve(2 * N));
    SHQ_TRY(ctx->yld_mark.reserve(2 * N));
    double *d_out = ctx->yld_out.ptr, *d_qout = ctx->yld_out.ptr + YOUT_NCOL * N;
    int32_t *d_slot = ctx->yld_i32.ptr, *d_qpos = ctx->yld_i32.ptr + N;
    uint8_t *d_mark = ctx->yld_mark.ptr, *d_flags = ctx->yld_mark.ptr + N;
    SHQ_HIP(hipMemcpyAsync(ctx->yld_in.ptr, hin.data(), sizeof(double) * hin.size(), hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(d_slot, hslot.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, st));
    const YieldDesc &d = ctx->yld_desc;
    const TimeTab tt = {ctx->yld_time.ptr, ctx->yld_time.ptr + ctx->yld_time_n, (long long) ctx->yld_time_n, ctx->yld_loga0, ctx->yld_dloga};
    const size_t lds = sizeof(double) * (size_t) d.ndoubles;
    hipEvent_t *eb = &ctx->ev_begin[SHQ_T_SPH], *ee = &ctx->ev_end[SHQ_T_SPH];
    SHQ_HIP(hipEventRecord(eb[0], st));
    yields_init_kernel<<<dim3(nblk(cnt)), dim3(256), lds, st>>>((long long) cnt, d, ctx->yld_tab.ptr, tt, atime, d_slot, ctx->yld_in.ptr, d_out, d_mark, d_flags);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipEventRecord(ee[0], st));
    /* the queue: the list positions with work, ascending = in active-list order (a stable selection, no atomic counter) */
    int64_t nq = 0;
    SHQ_TRY(shq_marked_list(ctx, d_mark, cnt, d_qpos, &nq));
    SHQ_HIP(hipEventRecord(eb[1], st));
    if(nq > 0) {
        yields_queue_kernel<<<dim3(nblk(nq)), dim3(256), lds, st>>>((long long) nq, (long long) cnt, d, ctx->yld_tab.ptr, d_qpos, ctx->yld_in.ptr, d_out, d_qout);
        SHQ_HIP(hipGetLastError());
    }
    SHQ_HIP(hipEventRecord(ee[1], st));
    std::vector<double> hout(YOUT_NCOL * N);
    std::vector<uint8_t> hflags(N);
    std::vector<int32_t> hqpos((size_t) std::max<int64_t>(nq, 1));
    SHQ_HIP(hipMemcpyAsync(hout.data(), d_out, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipMemcpyAsync(hflags.data(), d_flags, N, hipMemcpyDeviceToHost, st));
    if(nq > 0) {
        SHQ_HIP(hipMemcpyAsync(hqpos.data(), d_qpos, sizeof(int32_t) * (size_t) nq, hipMemcpyDeviceToHost, st));
        SHQ_HIP(hipMemcpyAsync(MassGenerated, d_qout, sizeof(double) * (size_t) nq, hipMemcpyDeviceToHost, st));
        SHQ_HIP(hipMemcpyAsync(MetalGenerated, d_qout + nq, sizeof(double) * (size_t) nq, hipMemcpyDeviceToHost, st));
        SHQ_HIP(hipMemcpyAsync(MetalSpeciesGenerated, d_qout + 2 * nq, sizeof(double) * (size_t) nq * SHQ_YIELD_NMETALS, hipMemcpyDeviceToHost, st));
    }
    SHQ_HIP(hipStreamSynchronize(st));
    for(int j = 0; j < 2; j++) {
        float ms = 0;
        SHQ_HIP(hipEventElapsedTime(&ms, eb[j], ee[j]));
        ctx->yld_ms[j] = ms;
    }
    for(int64_t k = 0; k < cnt; k++) {
        const int32_t pi = hslot[(size_t) k];
        if(pi < 0)
            continue;
        StellarAges[pi] = hout[YOUT_AGE * N + k];
        LowDyingMass[pi] = hout[YOUT_LOW * N + k];
        HighDyingMass[pi] = hout[YOUT_HIGH * N + k];
        MassReturn[pi] = hout[YOUT_MASSRETURN * N + k];
        if(hflags[(size_t) k] & YFLAG_REWRITTEN) /* "Ensure that we skip this step" (:453-455) */
            *sfield<float>(stars, pi, stars->off_lastenrichmentmyr) = (float) hout[YOUT_LASTENRICH * N + k];
    }
    for(int64_t q = 0; q < nq; q++) {
        const int64_t k = hqpos[(size_t) q];
        queue[q] = (int32_t) (active ? active[k] : k);
    }
    *nqueue = nq;
    return SHQ_OK;
}

extern "C" int shq_metal_yields_last_ms(shq_context *ctx, double ms[2])
{
    SHQ_CHECK(ctx && ms, SHQ_ERR_INVALID, "null argument");
    ms[0] = ctx->yld_ms[0];
    ms[1] = ctx->yld_ms[1];
    return SHQ_OK;
}

extern "C" int shq_metal_return_postprocess(shq_context *ctx, const shq_part_view *parts, const shq_star_yield_view *stars, const int32_t *queue, int64_t nqueue,
                                            const double *MassReturn, const double *StellarAges)
{
    SHQ_CHECK(ctx && parts && stars && (nqueue == 0 || (queue && MassReturn && StellarAges)), SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(parts->off_mass != SHQ_NOFIELD && parts->off_type != SHQ_NOFIELD && parts->off_pi != SHQ_NOFIELD, SHQ_ERR_INVALID,
              "metal_return_postprocess: the particle view needs Mass, Type and PI");
    SHQ_CHECK(nqueue >= 0, SHQ_ERR_INVALID, "metal_return_postprocess: negative queue length");
    SHQ_TRY(shq_walk_check_status(ctx, false));
    if(nqueue == 0)
        return SHQ_OK;
    const int64_t n = parts->numpart;
    const size_t NQ = (size_t) nqueue;
    std::vector<double> rows(4 * NQ);
    std::vector<int32_t> hslot(NQ);
    for(int64_t q = 0; q < nqueue; q++) {
        const int64_t i = queue[q];
        SHQ_CHECK(i >= 0 && i < n && *pfield<uint8_t>(parts, i, parts->off_type) == 4, SHQ_ERR_INVALID, "metal_return_postprocess: queue[%ld] = %ld is not a star", (long) q,
                  (long) i);
        const int32_t pi = *pfield<int32_t>(parts, i, parts->off_pi);
        SHQ_CHECK(pi >= 0 && pi < stars->numslots, SHQ_ERR_INVALID, "metal_return_postprocess: star %ld has PI %d outside the slot array", (long) i, pi);
        hslot[(size_t) q] = pi;
        rows[q] = (double) *pfield<float>(parts, i, parts->off_mass);
        rows[NQ + q] = *sfield<double>(stars, pi, stars->off_totalmassreturned);
        rows[2 * NQ + q] = MassReturn[q];
        rows[3 * NQ + q] = StellarAges[pi];
    }
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SHQ_TRY(ctx->yld_out.reserve(4 * NQ));
    SHQ_TRY(ctx->yld_i32.reserve(NQ));
    SHQ_HIP(hipMemcpyAsync(ctx->yld_out.ptr, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(ctx->yld_i32.ptr, queue, sizeof(int32_t) * NQ, hipMemcpyHostToDevice, st));
    /* the context's copy of these very particles follows the masses; laxer than parts_resident on purpose: a copy that is not vouched
     * for is uploaded again before anybody reads it, and the masses need no types */
    const bool resident = ctx->have_parts && ctx->cur_parts == parts->base && ctx->cur_parts_n == n && ctx->numpart == n;
    yields_postprocess_kernel<<<dim3(nblk(nqueue)), dim3(256), 0, st>>>((long long) nqueue, ctx->yld_i32.ptr, ctx->yld_out.ptr, resident ? ctx->posm.ptr : nullptr);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipMemcpyAsync(rows.data(), ctx->yld_out.ptr, sizeof(double) * rows.size(), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    for(int64_t q = 0; q < nqueue; q++) {
        const int64_t i = queue[q];
        const int32_t pi = hslot[(size_t) q];
        *reinterpret_cast<float *>(static_cast<char *>(parts->base) + (size_t) i * parts->elsize + parts->off_mass) = (float) rows[q];
        *sfield<double>(stars, pi, stars->off_totalmassreturned) = rows[NQ + q];
        *sfield<float>(stars, pi, stars->off_lastenrichmentmyr) = (float) rows[3 * NQ + q];
    }
    return SHQ_OK;
}
