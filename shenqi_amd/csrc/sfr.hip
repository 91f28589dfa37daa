/* sfr.hip — the star-forming branch on the device (include/shenqi_hip.h, "star formation"): the kernel that drives the
 * engine of sfr_math.hpp and the array-level entry shq_sfr_eval (the host entry shq_sfr_eval_host is in sfr_host.hip).
 *
 * One particle per lane, shaped like cooling.hip: a workgroup owns `chunk` consecutive entries of the list and hands them out through a
 * counter in LDS, so a lane whose particle has finished takes the next.  A particle needs between no solve at all and three long ones,
 * so the spread between lanes is wider than in the cooling kernel.  With refill off the share is one particle per lane.  Every particle
 * is written by exactly one lane, so which lane takes which particle changes no result.  The inputs of a particle are read again from
 * global memory whenever one of its solves ends, instead of being carried in registers through the solve. */
#include "common.hpp"
#include "sfr_math.hpp"
#include "cooling_uvbg.hpp"
#include <string.h>
#include <algorithm>

int shq_sfr_check_args(const shq_sfr_params *par, int what, int64_t n, const shq_sfr_arrays *in, const shq_sfr_eval_step *step, const double *out,
                       const uint8_t *flags_out, const uint8_t *decision, const uint8_t *branch, const int32_t *status);
SfrStep shq_sfr_engine_step(const shq_sfr_eval_step *step, int what, const double *rnd);

namespace {

enum { SFR_CHUNK_REFILL = 2048, SFR_CHUNK_PLAIN = 256 };
enum { SFR_IN_DENSITY = 0, SFR_IN_ENTROPY, SFR_IN_NE, SFR_IN_METALLICITY, SFR_IN_MASS, SFR_IN_HSML, SFR_IN_DIVVEL, SFR_IN_CURLVEL, SFR_IN_GRADRHO, SFR_IN_DLOGA,
       SFR_IN_DELAYTIME, SFR_IN_N };

struct DevSink {
    double *out; /* column k of [SHQ_SFR_NOUT][n] */
    uint8_t *f, *d, *b;
    size_t n;
    __device__ void put(int row, double x) { out[(size_t) row * n] = x; }
    __device__ double get(int row) const { return out[(size_t) row * n]; }
    __device__ void bytes(uint8_t flags, uint8_t decision, uint8_t branch)
    {
        *f = flags;
        *d = decision;
        *b = branch;
    }
};

struct EvalSrc {
    const double *in;  /* [SFR_IN_N][n] */
    const unsigned long long *ids;
    const uint8_t *timebin, *flags;
    double *out;       /* [SHQ_SFR_NOUT][n] */
    uint8_t *flags_out, *decision, *branch;
    int32_t *status, *steps;
    size_t n;
    CoolUV uv;
    __device__ SfrPart part(long long k) const
    {
        SfrPart p;
        p.Density = in[SFR_IN_DENSITY * n + k];
        p.Entropy = in[SFR_IN_ENTROPY * n + k];
        p.Ne = in[SFR_IN_NE * n + k];
        p.Metallicity = in[SFR_IN_METALLICITY * n + k];
        p.Mass = in[SFR_IN_MASS * n + k];
        p.Hsml = in[SFR_IN_HSML * n + k];
        p.DivVel = in[SFR_IN_DIVVEL * n + k];
        p.CurlVel = in[SFR_IN_CURLVEL * n + k];
        p.GradRho = in[SFR_IN_GRADRHO * n + k];
        p.dloga = in[SFR_IN_DLOGA * n + k];
        p.DelayTime = in[SFR_IN_DELAYTIME * n + k];
        p.ID = ids[k];
        p.timebin = timebin[k];
        p.flags = flags[k];
        return p;
    }
    __device__ void local_uvbg(long long, CoolUV &u_) const { u_ = uv; }
    __device__ DevSink sink(long long k) const { return DevSink{out + k, flags_out + k, decision + k, branch + k, n}; }
    __device__ void store(long long k, const SfrState &S) const
    {
        status[k] = S.status;
        steps[k] = S.steps;
    }
};

/* the particles of shq_starformation and shq_sfr_on_eeqos: the context's per-particle arrays */
struct PartSrc {
    SfrPartArgs a;
    __device__ SfrPart part(long long k) const
    {
        const long long i = a.list[k];
        const uint8_t fl = a.pflags[i];
        SfrPart p;
        p.Density = a.density[i];
        p.Entropy = a.entropy[i];
        p.Ne = a.ne[i];
        p.Metallicity = a.metallicity[i];
        /* not gas, garbage or swallowed (sfr_eff.cpp:238): Mass 0 makes the engine refuse the particle */
        p.Mass = ((fl >> 4) == 0 && !(fl & 1u)) ? a.posm[i].w : 0.0;
        p.Hsml = a.hsml[i];
        p.DivVel = a.divvel[i];
        p.CurlVel = a.curlvel[i];
        p.GradRho = a.gradrho ? a.gradrho[i] : 0.0;
        const int bin = a.bin[i];
        p.dloga = a.dloga_for_bin[bin];
        p.DelayTime = a.delaytime[i];
        p.ID = a.ids ? a.ids[i] : 0;
        p.timebin = bin;
        p.flags = a.flags[i];
        return p;
    }
    __device__ void local_uvbg(long long k, CoolUV &uv) const { cool_local_uvbg(a, (long long) a.list[k], uv); }
    __device__ DevSink sink(long long k) const { return DevSink{a.out + k, a.flags_out + k, a.decision + k, a.branch + k, a.cnt}; }
    __device__ void store(long long k, const SfrState &S) const
    {
        a.status[k] = S.status;
        a.steps[k] = S.steps;
    }
};

template <class Src>
__global__ __launch_bounds__(256) void sfr_kernel(Src src, SfrPar sp, CoolPar P, CoolTabs T, SfrStep st, long long n, int chunk, unsigned long long *stepsum)
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
    SfrState S;
    CoolUV uv; /* of the running solve */
    long long k = 0;
    bool have = false;
    unsigned long long mysteps = 0;
    auto set_uv = [&]() { /* a solve has begun: the global UVBG, or the particle's own */
        if(S.stage == SFR_SG_DONE)
            return;
        if(S.use_global)
            uv = st.global;
        else
            src.local_uvbg(k, uv);
    };
    auto fetch = [&]() {
        k = begin + atomicAdd(&s_next, 1);
        have = k < end;
        if(have) {
            const SfrPart p = src.part(k);
            DevSink sink = src.sink(k);
            sfr_begin(S, sp, P, st, p, sink);
            set_uv();
        }
    };
    fetch();
    while(__any(have)) {
        if(have) {
            if(S.stage != SFR_SG_DONE) {
                if(S.C.phase != COOL_PH_DONE)
                    cool_step(S.C, P, T, uv, S.in);
                if(S.C.phase == COOL_PH_DONE) {
                    const SfrPart p = src.part(k);
                    DevSink sink = src.sink(k);
                    sfr_advance(S, sp, P, st, p, sink);
                    set_uv();
                }
            }
            if(S.stage == SFR_SG_DONE) {
                src.store(k, S);
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

template <class Src> int launch_sfr(shq_context *ctx, const Src &src, const SfrPar &sp, const SfrStep &step, int64_t n)
{
    hipStream_t st = ctx->stream;
    SHQ_TRY(ctx->cool_cnt.reserve(1));
    SHQ_HIP(hipMemsetAsync(ctx->cool_cnt.ptr, 0, sizeof(unsigned long long), st));
    const int chunk = ctx->sfr_refill ? SFR_CHUNK_REFILL : SFR_CHUNK_PLAIN;
    const CoolTabs T{ctx->cool_ion.ptr, ctx->cool_rates.ptr, ctx->cool_par.metal_on ? ctx->cool_metal.ptr : nullptr};
    hipEvent_t eb = ctx->ev_begin[SHQ_T_SPH], ee = ctx->ev_end[SHQ_T_SPH];
    SHQ_HIP(hipEventRecord(eb, st));
    if(n > 0)
        sfr_kernel<Src><<<dim3(nblk(n, chunk)), dim3(256), 0, st>>>(src, sp, ctx->cool_par, T, step, (long long) n, chunk, ctx->cool_cnt.ptr);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipEventRecord(ee, st));
    unsigned long long h = 0;
    SHQ_HIP(hipMemcpyAsync(&h, ctx->cool_cnt.ptr, sizeof(h), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    float ms = 0;
    SHQ_HIP(hipEventElapsedTime(&ms, eb, ee));
    ctx->sfr_ms = ms;
    ctx->sfr_steps = (int64_t) h;
    return SHQ_OK;
}

} // namespace

int shq_sfr_run_device(shq_context *ctx, const SfrPartArgs *a, const shq_sfr_params *par, const SfrStep *step, int64_t cnt)
{
    PartSrc src;
    src.a = *a;
    return launch_sfr(ctx, src, *par, *step, cnt);
}

extern "C" int shq_sfr_set_refill(shq_context *ctx, int on)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    ctx->sfr_refill = on ? 1 : 0;
    return SHQ_OK;
}

extern "C" int shq_sfr_last_kernel(shq_context *ctx, double *ms, int64_t *steps)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    if(ms)
        *ms = ctx->sfr_ms;
    if(steps)
        *steps = ctx->sfr_steps;
    return SHQ_OK;
}

extern "C" int shq_sfr_eval(shq_context *ctx, const shq_sfr_params *par, int what, int64_t n, const shq_sfr_arrays *in, const shq_sfr_eval_step *step, double *out,
                            uint8_t *flags_out, uint8_t *decision, uint8_t *branch, int32_t *status, int32_t *steps)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    SHQ_TRY(shq_sfr_check_args(par, what, n, in, step, out, flags_out, decision, branch, status));
    SHQ_CHECK(ctx->cool_have, SHQ_ERR_STATE, "sfr_eval: shq_cooling_set_tables first");
    if(n == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t N = (size_t) n;
    /* the inputs, the outputs and the IDs (64 bits each, as the doubles): the context's bhw_ids is its copy of the caller's IDs by
     * particle index (ids_upload, SHQ_CURRENT_IDS) and is not this call's to overwrite */
    SHQ_TRY(ctx->cool_d.reserve((SFR_IN_N + SHQ_SFR_NOUT + 1) * N));
    SHQ_TRY(ctx->cool_i.reserve(2 * N));
    SHQ_TRY(ctx->cool_b.reserve(5 * N));
    SHQ_TRY(ctx->bhw_rnd.reserve((size_t) step->rnd_size));
    double *d = ctx->cool_d.ptr;
    uint8_t *b = ctx->cool_b.ptr;
    const double *src_in[SFR_IN_N] = {in->Density, in->Entropy, in->Ne,      in->Metallicity, in->Mass,     in->Hsml,
                                      in->DivVel,  in->CurlVel, in->GradRho, in->dloga,       in->DelayTime};
    for(int r = 0; r < SFR_IN_N; r++) {
        if(src_in[r])
            SHQ_HIP(hipMemcpyAsync(d + r * N, src_in[r], sizeof(double) * N, hipMemcpyHostToDevice, st));
        else
            SHQ_HIP(hipMemsetAsync(d + r * N, 0, sizeof(double) * N, st));
    }
    SHQ_HIP(hipMemsetAsync(d + SFR_IN_N * N, 0, sizeof(double) * SHQ_SFR_NOUT * N, st));
    SHQ_HIP(hipMemcpyAsync(b, in->timebin, N, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(b + N, in->flags, N, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemsetAsync(b + 2 * N, 0, 3 * N, st));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "ID width");
    static_assert(sizeof(unsigned long long) == sizeof(double), "IDs share the doubles' buffer");
    unsigned long long *d_ids = reinterpret_cast<unsigned long long *>(d + (SFR_IN_N + SHQ_SFR_NOUT) * N);
    SHQ_HIP(hipMemcpyAsync(d_ids, in->ID, sizeof(uint64_t) * N, hipMemcpyHostToDevice, st));
    SHQ_HIP(hipMemcpyAsync(ctx->bhw_rnd.ptr, step->rnd_table, sizeof(double) * (size_t) step->rnd_size, hipMemcpyHostToDevice, st));
    EvalSrc src;
    src.in = d;
    src.ids = d_ids;
    src.timebin = b;
    src.flags = b + N;
    src.out = d + SFR_IN_N * N;
    src.flags_out = b + 2 * N;
    src.decision = b + 3 * N;
    src.branch = b + 4 * N;
    src.status = ctx->cool_i.ptr;
    src.steps = ctx->cool_i.ptr + N;
    src.n = N;
    src.uv = shq_cooling_uv(&step->LocalUVBG);
    const SfrStep es = shq_sfr_engine_step(step, what, ctx->bhw_rnd.ptr);
    SHQ_TRY(launch_sfr(ctx, src, *par, es, n));
    std::vector<double> hout(SHQ_SFR_NOUT * N);
    std::vector<uint8_t> hb(3 * N);
    std::vector<int32_t> hsteps(N);
    SHQ_HIP(hipMemcpyAsync(hout.data(), src.out, sizeof(double) * hout.size(), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipMemcpyAsync(hb.data(), b + 2 * N, 3 * N, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipMemcpyAsync(status, ctx->cool_i.ptr, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipMemcpyAsync(hsteps.data(), ctx->cool_i.ptr + N, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    for(size_t k = 0; k < N; k++) {
        if(steps)
            steps[k] = hsteps[k];
        if(status[k] != COOL_ST_OK)
            continue;
        for(size_t r = 0; r < SHQ_SFR_NOUT; r++)
            out[r * N + k] = hout[r * N + k];
        flags_out[k] = hb[k];
        decision[k] = hb[N + k];
        branch[k] = hb[2 * N + k];
    }
    return SHQ_OK;
}
