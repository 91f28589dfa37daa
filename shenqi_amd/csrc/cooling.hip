/* cooling.hip — radiative cooling on the device (include/shenqi_hip.h, "radiative cooling"): the kernels that drive the
 * engine of cooling_math.hpp, the table upload, the array-level queries on the device, and the device half of shq_cooling (its host
 * half, which gathers and writes back the caller's records, is in sph_capi.hip; the host entry shq_cooling_eval_host in cooling_host.hip).
 *
 * One particle per lane.  A workgroup owns `chunk` consecutive entries of the list and hands them out through a counter in LDS: a lane
 * whose particle has finished stores it and takes the next, so a wave ends when its workgroup's share is used up, not when the slowest
 * of its first 64 particles is.  With refill off the share is one particle per lane.  Every particle is independent and written by
 * exactly one lane, so which lane takes which particle changes no result. */
#include "common.hpp"
#include "cooling_uvbg.hpp"
#include <string.h>
#include <algorithm>

namespace {

enum { COOL_CHUNK_REFILL = 2048, COOL_CHUNK_PLAIN = 256 };

struct EvalSrc {
    const double *rho, *u, *Z, *dt;
    const uint8_t *heiii;
    double *ne, *out;
    int32_t *status, *steps;
    CoolUV uv;
    double redshift, min_egy_spec, lmfp;
    int what;
    __device__ void load(const CoolPar &P, long long k, CoolIn &in, CoolUV &u_, CoolState &S) const
    {
        cool_eval_in(P, what, rho[k], u[k], Z ? Z[k] : 0.0, heiii ? heiii[k] : 0, dt ? dt[k] : 0.0, redshift, min_egy_spec, lmfp, &in);
        u_ = uv;
        cool_init(S, in, ne[k]);
    }
    __device__ void store(const CoolPar &P, long long k, const CoolIn &in, const CoolState &S) const
    {
        status[k] = S.status;
        steps[k] = S.steps;
        if(S.status != COOL_ST_OK)
            return;
        out[k] = cool_eval_out(P, what, S.out);
        if(cool_eval_updates_ne(what))
            ne[k] = S.ne_guess;
    }
};

/* cooling_direct (sfr_eff.cpp:430-481) on the context's per-particle arrays */
struct PartSrc {
    CoolPartArgs a;
    __device__ double enttou(long long i) const { return exp(SHQ_COOL_GAMMA_MINUS1 * log(a.density[i] * a.a3inv)) / SHQ_COOL_GAMMA_MINUS1; }
    __device__ void local_uvbg(long long i, CoolUV &uv) const { cool_local_uvbg(a, i, uv); }
    __device__ void load(const CoolPar &P, long long k, CoolIn &in, CoolUV &uv, CoolState &S) const
    {
        const long long i = a.list[k];
        const int bin = a.bin[i];
        const double dtime = a.dloga_for_bin[bin] / a.hubble;
        const double e2u = enttou(i);
        const double uold = a.entropy[i] * e2u;
        local_uvbg(i, uv);
        const double lastred = a.lastred_for_bin[bin];
        const int heiii = (a.pflags[i] & SHQ_FLAG_HEIII) ? 1 : 0;
        const double mw_neutral = 4.0 / (1 + 3 * 0.76);
        cool_eval_in(P, COOL_WHAT_UNEW, a.density[i] * a.a3inv, uold, a.metallicity[i], heiii, dtime, a.redshift, a.temp_to_u / mw_neutral * a.MinGasTemp, a.lmfp, &in);
        cool_init(S, in, a.ne[i]);
        if(S.phase != COOL_PH_DONE && a.HIReionTemp > 0 && uv.zreion >= a.redshift && uv.zreion < lastred) {
            /* reionised this step: the HI reionisation temperature with singly ionised helium (:455-468) */
            const double meanweight = 4 / (8 - 6 * (1 - 0.76));
            double unew = a.temp_to_u / meanweight * a.HIReionTemp;
            if(uold > unew)
                unew = uold;
            cool_finish(S, COOL_ST_OK, unew * P.uu_in_cgs);
            S.ne_guess = a.ne[i];
            S.stage = 2; /* the bump: store takes unew as it stands */
            S.u = unew;
        }
    }
    __device__ void store(const CoolPar &P, long long k, const CoolIn &in, const CoolState &S) const
    {
        const long long i = a.list[k];
        a.status[k] = S.status;
        a.steps[k] = S.steps;
        if(S.status != COOL_ST_OK)
            return;
        const double unew = S.stage == 2 ? S.u : S.out / P.uu_in_cgs;
        a.entropy[i] = unew / enttou(i);
        a.ne[i] = S.ne_guess;
    }
};

template <class Src> __global__ __launch_bounds__(256) void cooling_kernel(Src src, CoolPar P, CoolTabs T, long long n, int chunk, unsigned long long *stepsum)
{
    __shared__ int s_next;
    __shared__ unsigned long long s_steps;
    const long long begin = (long long) blockIdx.x * chunk;
    const long long end = begin + chunk < n ? begin + chunk : n;
    if(threadIdx.x == 0) {
        s_next = 0;
        s_steps = 0;
    }
    __syncthreads();
    CoolState S;
    CoolIn in;
    CoolUV uv;
    long long k = 0;
    bool have = false;
    unsigned long long mysteps = 0;
    auto fetch = [&]() {
        k = begin + atomicAdd(&s_next, 1);
        have = k < end;
        if(have)
            src.load(P, k, in, uv, S);
    };
    fetch();
    while(__any(have)) {
        if(have) {
            if(S.phase != COOL_PH_DONE)
                cool_step(S, P, T, uv, in);
            if(S.phase == COOL_PH_DONE) {
                src.store(P, k, in, S);
                mysteps += (unsigned long long) S.steps;
                fetch();
            }
        }
    }
    atomicAdd(&s_steps, mysteps);
    __syncthreads();
    if(threadIdx.x == 0)
        atomicAdd(stepsum, s_steps);
}

/* shq_cooling's first pass, by list position: 1 cool, 2 on the effective equation of state, 0 skipped (sfr_eff.cpp:238, :502-517) */
__global__ void cooling_classify_kernel(long long cnt, const int32_t *__restrict__ list, const uint8_t *__restrict__ pflags, const double4 *__restrict__ posm,
                                        const double *__restrict__ density, const double *__restrict__ delay, const uint8_t *__restrict__ mask, int StarformationOn,
                                        double PhysDensThresh, double OverDensThresh, double a3inv, uint8_t *mark_cool, uint8_t *mark_eeqos)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= cnt)
        return;
    const long long i = list ? (long long) list[k] : k;
    const uint8_t fl = pflags[i];
    uint8_t c = 0, e = 0;
    if((fl >> 4) == 0 && !(fl & 1u) && posm[i].w > 0) {
        int flag = 0;
        if(mask)
            flag = mask[i] != 0;
        else if(StarformationOn) {
            if(density[i] * a3inv >= PhysDensThresh)
                flag = 1;
            if(density[i] < OverDensThresh)
                flag = 0;
            if(delay[i] > 0)
                flag = 0;
        }
        c = flag ? 0 : 1;
        e = flag ? 1 : 0;
    }
    mark_cool[k] = c;
    mark_eeqos[k] = e;
}
__global__ void cooling_positions_kernel(long long m, const int32_t *__restrict__ list, int32_t *pos)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t < m && list)
        pos[t] = list[pos[t]];
}

template <class Src> int launch_cooling(shq_context *ctx, const Src &src, int64_t n)
{
    hipStream_t st = ctx->stream;
    SHQ_TRY(ctx->cool_cnt.reserve(1));
    SHQ_HIP(hipMemsetAsync(ctx->cool_cnt.ptr, 0, sizeof(unsigned long long), st));
    const int chunk = ctx->cool_refill ? COOL_CHUNK_REFILL : COOL_CHUNK_PLAIN;
    const CoolTabs T{ctx->cool_ion.ptr, ctx->cool_rates.ptr, ctx->cool_par.metal_on ? ctx->cool_metal.ptr : nullptr};
    hipEvent_t eb = ctx->ev_begin[SHQ_T_SPH], ee = ctx->ev_end[SHQ_T_SPH];
    SHQ_HIP(hipEventRecord(eb, st));
    if(n > 0)
        cooling_kernel<Src><<<dim3(nblk(n, chunk)), dim3(256), 0, st>>>(src, ctx->cool_par, T, (long long) n, chunk, ctx->cool_cnt.ptr);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipEventRecord(ee, st));
    unsigned long long h = 0;
    SHQ_HIP(hipMemcpyAsync(&h, ctx->cool_cnt.ptr, sizeof(h), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    float ms = 0;
    SHQ_HIP(hipEventElapsedTime(&ms, eb, ee));
    ctx->cool_ms = ms;
    ctx->cool_steps = (int64_t) h;
    return SHQ_OK;
}

template <typename T> int upload(shq_context *ctx, DevBuf<T> &b, const T *h, size_t n)
{
    SHQ_TRY(b.reserve(std::max<size_t>(n, 1)));
    if(n > 0)
        SHQ_HIP(hipMemcpyAsync(b.ptr, h, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream));
    return SHQ_OK;
}

} // namespace

extern "C" int shq_cooling_set_tables(shq_context *ctx, const shq_cooling_tables *t)
{
    SHQ_CHECK(ctx && t, SHQ_ERR_INVALID, "null argument");
    CoolPar P;
    std::vector<double> ion, rates;
    SHQ_TRY(shq_cooling_tables_to_engine(t, &P, &ion, &rates));
    SHQ_CHECK(!t->zreion || (t->zreion_nside >= 2 && t->zreion_nside <= 2048 && std::isfinite(t->zreion_boxsize) && t->zreion_boxsize > 0), SHQ_ERR_INVALID,
              "cooling: Zreion table with Nside = %d, BoxSize = %g", t->zreion_nside, t->zreion_boxsize);
    SHQ_HIP(hipSetDevice(ctx->device));
    ctx->cool_have = false;
    SHQ_TRY(upload(ctx, ctx->cool_ion, ion.data(), ion.size()));
    SHQ_TRY(upload(ctx, ctx->cool_rates, rates.data(), rates.size()));
    if(t->metal)
        SHQ_TRY(upload(ctx, ctx->cool_metal, t->metal, (size_t) t->metal_dims[0] * t->metal_dims[1] * t->metal_dims[2]));
    ctx->cool_znside = 0;
    if(t->zreion) {
        const size_t ns = (size_t) t->zreion_nside;
        SHQ_TRY(upload(ctx, ctx->cool_zreion, t->zreion, ns * ns * ns));
        ctx->cool_znside = t->zreion_nside;
        ctx->cool_zbox = t->zreion_boxsize;
    }
    SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* the uploads read the caller's and this frame's memory */
    ctx->cool_par = P;
    ctx->cool_fbar = t->fBar;
    ctx->cool_have = true;
    return SHQ_OK;
}

extern "C" int shq_cooling_set_refill(shq_context *ctx, int on)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    ctx->cool_refill = on ? 1 : 0;
    return SHQ_OK;
}

extern "C" int shq_cooling_last_kernel(shq_context *ctx, double *ms, int64_t *steps)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    if(ms)
        *ms = ctx->cool_ms;
    if(steps)
        *steps = ctx->cool_steps;
    return SHQ_OK;
}

extern "C" int shq_cooling_eval(shq_context *ctx, int what, int64_t n, const double *rho, const double *u, double *ne, const double *Z, const uint8_t *heiii,
                                const double *dt, const shq_cooling_uvbg *uvbg, double redshift, double min_egy_spec, double lmfp_heat, double *out, int32_t *status,
                                int32_t *steps)
{
    SHQ_CHECK(ctx && uvbg && n >= 0 && (n == 0 || (rho && u && ne && out && status)), SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(what >= 0 && what < COOL_WHAT_N, SHQ_ERR_INVALID, "cooling_eval: what = %d", what);
    SHQ_CHECK(what != COOL_WHAT_UNEW || n == 0 || dt, SHQ_ERR_INVALID, "cooling_eval: UNEW needs dt");
    SHQ_CHECK(n < (1ll << 31), SHQ_ERR_INVALID, "cooling_eval: too many particles");
    SHQ_CHECK(ctx->cool_have, SHQ_ERR_STATE, "cooling_eval: shq_cooling_set_tables first");
    if(n == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t N = (size_t) n;
    /* rho, u, ne, Z, dt, out */
    SHQ_TRY(ctx->cool_d.reserve(6 * N));
    SHQ_TRY(ctx->cool_i.reserve(2 * N));
    SHQ_TRY(ctx->cool_b.reserve(N));
    double *d = ctx->cool_d.ptr;
    SHQ_HIP(hipMemcpyAsync(d, rho, sizeof(double) * N, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(d + N, u, sizeof(double) * N, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(d + 2 * N, ne, sizeof(double) * N, hipMemcpyHostToDevice, st));
    if(Z)
        SHQ_HIP(hipMemcpyAsync(d + 3 * N, Z, sizeof(double) * N, hipMemcpyHostToDevice, st));
    if(dt)
        SHQ_HIP(hipMemcpyAsync(d + 4 * N, dt, sizeof(double) * N, hipMemcpyHostToDevice, st));
    if(heiii)
        SHQ_HIP(hipMemcpyAsync(ctx->cool_b.ptr, heiii, N, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemsetAsync(d + 5 * N, 0, sizeof(double) * N, st));
    EvalSrc src;
    src.rho = d;
    src.u = d + N;
    src.ne = d + 2 * N;
    src.Z = Z ? d + 3 * N : nullptr;
    src.dt = dt ? d + 4 * N : nullptr;
    src.heiii = heiii ? ctx->cool_b.ptr : nullptr;
    src.out = d + 5 * N;
    src.status = ctx->cool_i.ptr;
    src.steps = ctx->cool_i.ptr + N;
    src.uv = shq_cooling_uv(uvbg);
    src.redshift = redshift;
    src.min_egy_spec = min_egy_spec;
    src.lmfp = lmfp_heat;
    src.what = what;
    SHQ_TRY(launch_cooling(ctx, src, n));
    std::vector<double> hout(N), hne(N);
    SHQ_HIP(hipMemcpyAsync(hout.data(), d + 5 * N, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipMemcpyAsync(hne.data(), d + 2 * N, sizeof(double) * N, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipMemcpyAsync(status, ctx->cool_i.ptr, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    if(steps)
        SHQ_HIP(hipMemcpyAsync(steps, ctx->cool_i.ptr + N, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    for(size_t k = 0; k < N; k++)
        if(status[k] == COOL_ST_OK) {
            out[k] = hout[k];
            ne[k] = hne[k];
        }
    return SHQ_OK;
}

/* ---- the device half of shq_cooling ------------------------------------------------------------------------------------------------ */

int shq_cooling_classify_device(shq_context *ctx, const int32_t *d_list, int64_t cnt, const uint8_t *d_mask, int StarformationOn, double PhysDensThresh,
                                double OverDensThresh, double a3inv, int32_t *d_cool, int64_t *ncool, int32_t *d_eeqos, int64_t *neeqos)
{
    *ncool = *neeqos = 0;
    if(cnt <= 0)
        return SHQ_OK;
    SHQ_TRY(ctx->cool_b.reserve(2 * (size_t) cnt));
    uint8_t *mc = ctx->cool_b.ptr, *me = mc + cnt;
    cooling_classify_kernel<<<dim3(nblk(cnt)), dim3(256), 0, ctx->stream>>>((long long) cnt, d_list, ctx->pflags.ptr, ctx->posm.ptr, ctx->g_density.ptr,
                                                                            ctx->g_delaytime.ptr, d_mask, StarformationOn, PhysDensThresh, OverDensThresh, a3inv, mc, me);
    SHQ_HIP(hipGetLastError());
    /* stable selections: both lists come out in list order */
    SHQ_TRY(shq_marked_list(ctx, mc, cnt, d_cool, ncool));
    SHQ_TRY(shq_marked_list(ctx, me, cnt, d_eeqos, neeqos));
    if(d_list) {
        if(*ncool > 0)
            cooling_positions_kernel<<<dim3(nblk(*ncool)), dim3(256), 0, ctx->stream>>>((long long) *ncool, d_list, d_cool);
        if(*neeqos > 0)
            cooling_positions_kernel<<<dim3(nblk(*neeqos)), dim3(256), 0, ctx->stream>>>((long long) *neeqos, d_list, d_eeqos);
        SHQ_HIP(hipGetLastError());
    }
    return SHQ_OK;
}

int shq_cooling_run_device(shq_context *ctx, const CoolPartArgs *a, int64_t ncool)
{
    PartSrc src;
    src.a = *a;
    return launch_cooling(ctx, src, ncool);
}
