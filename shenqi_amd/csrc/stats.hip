/* stats.hip — the particle loops behind the run's log files (include/shenqi_hip.h, "Run logs").
 *
 *   compute_global_quantities_of_system's loop   stats.cpp:235-272    shq_energy_statistics
 *   its rank-0 block                             stats.cpp:289-361    shq_stats_finish (host)
 *   write_blackhole_txt's loop                   bhinfo.cpp:176-184   shq_bh_totals
 *   collect_BH_info's loop                       bhinfo.cpp:76-151    shq_bh_details
 *
 * The record pass is startup.hip's (record_tile.hpp): a workgroup stages ST_TILE records in LDS with 16-byte loads and lane k works on
 * record k there; nothing is written back.  The sums: per type present in the wave's ballot one butterfly over the wave (lanes of another
 * type add 0.0, which is exact), the four wave sums added in wave order, one partial per workgroup and column; a second kernel adds the
 * partials of a column in a fixed order.  No floating-point atomics, so equal inputs give equal bytes.
 * The temperature solves diverge and need the cooling engine's registers, so they do not live in the record pass: it marks the gas
 * particles, a stable selection turns the marks into a list, and a second kernel with one gas particle per lane solves and sums
 * Mass * T in the same fixed shape. */
#include "common.hpp"
#include "record_tile.hpp"
#include "cooling_uvbg.hpp"
#include <math.h>
#include <string.h>

namespace {

#define STAT_GAMMA_MINUS1 ((5.0 / 3.0) - 1) /* physconst.h:35-36; get_temp's helium, 1 - HYDROGEN_MASSFRAC, is the engine's SHQ_COOL_HELIUM */
constexpr int STAT_PER_TYPE = 12;                /* Mass, EnergyPot, EnergyKin, Momentum[3], AngMomentum[3], CenterOfMass[3] */
constexpr int STAT_EINT = 6 * STAT_PER_TYPE;     /* EnergyIntComp[0] */
constexpr int STAT_NCOL = STAT_EINT + 1;         /* columns of the record pass; TemperatureComp[0] has a pass of its own */
/* stat_cnt */
enum { SC_COUNT = 0 /* .. 5 */, SC_BADTYPE = 6, SC_BADPI, SC_STATUS /* .. + 3 */, SC_BH_NUM = SC_STATUS + SHQ_COOL_NSTATUS, SC_BH_BAD, SC_N };

/* what cool_local_uvbg reads, for one gas particle: the members carry CoolPartArgs' names (cooling_uvbg.hpp) */
struct StatOne {
    double v;
    __device__ double operator[](long long) const { return v; }
};
struct StatOnePos {
    double4 v;
    __device__ const double4 &operator[](long long) const { return v; }
};
struct StatUV {
    StatOnePos posm;
    StatOne j21, zre;
    const double *ztab;
    int znside, mode;
    double zbox, offset[3];
    CoolUV global;
    double j21c[6], ss_grey, ss_fbar;
    double redshift;
};

struct StatArgs {
    shq_stats_layout L;
    double a1, a2, a3;
    const char *parts, *sph;
    long long numpart, nsph;
    int wide;
    unsigned pitch, nblocks;
};

__global__ __launch_bounds__(ST_TILE) void stat_energy_kernel(StatArgs A, uint8_t *mark, unsigned long long *cnt, double *partial)
{
#pragma clang fp contract(off)
    extern __shared__ uint2 stat_tile_[];
    __shared__ double s_wsum[ST_TILE / 64][STAT_NCOL];
    __shared__ unsigned s_cnt[8];
    char *lds = reinterpret_cast<char *>(stat_tile_);
    const shq_stats_layout &L = A.L;
    const int k = threadIdx.x;
    const long long row0 = (long long) blockIdx.x * ST_TILE;
    const int nrow = (int) (A.numpart - row0 < ST_TILE ? A.numpart - row0 : ST_TILE);
    if(k < 8)
        s_cnt[k] = 0;
    const char *gtile = A.parts + (size_t) row0 * L.part_elsize;
    if(A.wide)
        st_stage_in<16>(lds, A.pitch, gtile, (unsigned) L.part_elsize, nrow);
    else
        st_stage_in<8>(lds, A.pitch, gtile, (unsigned) L.part_elsize, nrow);
    __syncthreads();
    const bool live = k < nrow;
    const char *rec = lds + (unsigned) (live ? k : 0) * A.pitch;
    const int type = live ? *reinterpret_cast<const uint8_t *>(rec + L.off_type) : -1;
    double v[STAT_PER_TYPE], eint = 0;
    bool badpi = false;
    {
        const double m = *reinterpret_cast<const float *>(rec + L.off_mass);
        const double *pos = reinterpret_cast<const double *>(rec + L.off_pos), *vel = reinterpret_cast<const double *>(rec + L.off_vel);
        const double pot = *reinterpret_cast<const double *>(rec + L.off_potential);
        v[0] = m;
        v[1] = 0.5 * m * pot / A.a1;
        v[2] = 0.5 * m * (vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]) / A.a2;
        for(int j = 0; j < 3; j++) {
            v[3 + j] = m * vel[j];
            v[9 + j] = m * pos[j];
        }
        v[6] = m * (pos[1] * vel[2] - pos[2] * vel[1]);
        v[7] = m * (pos[2] * vel[0] - pos[0] * vel[2]);
        v[8] = m * (pos[0] * vel[1] - pos[1] * vel[0]);
        if(type == 0) {
            const long long pi = *reinterpret_cast<const int32_t *>(rec + L.off_pi);
            badpi = pi < 0 || pi >= A.nsph;
            if(!badpi) {
                const char *s = A.sph + (size_t) pi * L.sph_elsize;
                const double entr = *reinterpret_cast<const double *>(s + L.sph_off_entropy);
                const double egyspec = entr / STAT_GAMMA_MINUS1 * pow(*reinterpret_cast<const double *>(s + L.sph_off_density) / A.a3, STAT_GAMMA_MINUS1);
                eint = m * egyspec;
            }
        }
    }
    if(mark && live)
        mark[row0 + k] = type == 0 && !badpi;
    const int w = k >> 6;
    const bool lane0 = (k & 63) == 0;
#pragma unroll
    for(int t = 0; t < 6; t++) {
        const unsigned long long present = shq_ballot(type == t);
        if(present == 0) { /* wave-uniform */
            if(lane0) {
                for(int c = 0; c < STAT_PER_TYPE; c++)
                    s_wsum[w][t * STAT_PER_TYPE + c] = 0;
                if(t == 0)
                    s_wsum[w][STAT_EINT] = 0;
            }
            continue;
        }
        double r[STAT_PER_TYPE + 1];
#pragma unroll
        for(int c = 0; c < STAT_PER_TYPE; c++)
            r[c] = type == t ? v[c] : 0.0;
        r[STAT_PER_TYPE] = t == 0 ? eint : 0.0; /* eint is 0 off type 0 */
        const int nc = t == 0 ? STAT_PER_TYPE + 1 : STAT_PER_TYPE;
#pragma unroll
        for(int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for(int c = 0; c < STAT_PER_TYPE + 1; c++)
                if(c < nc)
                    r[c] += __shfl_xor(r[c], off, 64);
        if(lane0) {
#pragma unroll
            for(int c = 0; c < STAT_PER_TYPE; c++)
                s_wsum[w][t * STAT_PER_TYPE + c] = r[c];
            if(t == 0)
                s_wsum[w][STAT_EINT] = r[STAT_PER_TYPE];
            atomicAdd(&s_cnt[t], (unsigned) __popcll((long long) present));
        }
    }
    const unsigned long long badtype = shq_ballot(type > 5), badpis = shq_ballot(badpi);
    if(lane0 && badtype)
        atomicAdd(&s_cnt[SC_BADTYPE], (unsigned) __popcll((long long) badtype));
    if(lane0 && badpis)
        atomicAdd(&s_cnt[SC_BADPI], (unsigned) __popcll((long long) badpis));
    __syncthreads();
    if(k < STAT_NCOL) {
        double s = s_wsum[0][k];
        for(int ww = 1; ww < ST_TILE / 64; ww++)
            s += s_wsum[ww][k];
        partial[(size_t) k * A.nblocks + blockIdx.x] = s;
    }
    if(k >= 128 && k < 136 && s_cnt[k - 128])
        atomicAdd(&cnt[k - 128], (unsigned long long) s_cnt[k - 128]);
}

/* column blockIdx.x of the block partials in a fixed order: thread j adds partials j, j + 256, ..., then a halving tree over the threads */
__global__ __launch_bounds__(256) void stat_final_sum_kernel(long long nblocks, const double *__restrict__ partial, double *out)
{
#pragma clang fp contract(off)
    __shared__ double s[256];
    const double *col = partial + (size_t) blockIdx.x * nblocks;
    double a = 0;
    for(long long b = threadIdx.x; b < nblocks; b += 256)
        a += col[b];
    s[threadIdx.x] = a;
    __syncthreads();
    for(int h = 128; h >= 1; h >>= 1) {
        if((int) threadIdx.x < h)
            s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if(threadIdx.x == 0)
        out[blockIdx.x] = s[0];
}

/* the sum of one value per lane in the fixed shape: butterfly, wave order, one partial per workgroup */
__device__ __forceinline__ void stat_block_sum(double x, double *s_w, double *partial)
{
#pragma clang fp contract(off)
    for(int off = 32; off >= 1; off >>= 1)
        x += __shfl_xor(x, off, 64);
    if((threadIdx.x & 63) == 0)
        s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    if(threadIdx.x == 0) {
        double s = s_w[0];
        for(unsigned w = 1; w < blockDim.x / 64; w++)
            s += s_w[w];
        partial[blockIdx.x] = s;
    }
    __syncthreads();
}

/* get_temp for the gas particle at list position k; Mass * T into the sum, the outcome into the counters, mark = the solve did not end OK */
__global__ __launch_bounds__(256) void stat_temperature_kernel(StatArgs A, StatUV U, CoolPar P, CoolTabs T, const int32_t *__restrict__ list, long long ngas,
                                                               uint8_t *mark, unsigned long long *cnt, double *partial)
{
#pragma clang fp contract(off)
    __shared__ double s_w[4];
    __shared__ unsigned s_cnt[SHQ_COOL_NSTATUS];
    const shq_stats_layout &L = A.L;
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(threadIdx.x < SHQ_COOL_NSTATUS)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    double mt = 0;
    int st = -1;
    if(k < ngas) {
        const char *rec = A.parts + (size_t) list[k] * L.part_elsize;
        const double m = *reinterpret_cast<const float *>(rec + L.off_mass);
        const long long pi = *reinterpret_cast<const int32_t *>(rec + L.off_pi);
        st = COOL_ST_BADINPUT;
        if(pi >= 0 && pi < A.nsph) { /* the record pass has checked it; the test keeps a broken caller inside the array */
            const char *s = A.sph + (size_t) pi * L.sph_elsize;
            const double dens = *reinterpret_cast<const double *>(s + L.sph_off_density), entr = *reinterpret_cast<const double *>(s + L.sph_off_entropy);
            const double egyspec = entr / STAT_GAMMA_MINUS1 * pow(dens / A.a3, STAT_GAMMA_MINUS1);
            const double *pos = reinterpret_cast<const double *>(rec + L.off_pos);
            U.posm.v = make_double4(pos[0], pos[1], pos[2], 0.0);
            if(U.mode == SHQ_COOL_UVBG_J21) {
                U.j21.v = *reinterpret_cast<const double *>(s + L.sph_off_local_j21);
                U.zre.v = *reinterpret_cast<const double *>(s + L.sph_off_zreion);
            }
            CoolUV uv;
            cool_local_uvbg(U, 0, uv);
            /* get_temp(Density, egyspec, 1 - HYDROGEN_MASSFRAC, &uvbg, &ne): internal units, as the reference passes them */
            CoolIn in;
            in.rho = dens;
            in.u_old = egyspec;
            in.dt = 0;
            in.Z = 0;
            in.minegy = 0;
            in.redshift = U.redshift;
            in.lmfp = 0;
            in.what = COOL_WHAT_TEMP;
            CoolState S;
            cool_init(S, in, *reinterpret_cast<const double *>(s + L.sph_off_ne));
            while(S.phase != COOL_PH_DONE)
                cool_step(S, P, T, uv, in);
            st = S.status;
            if(st == COOL_ST_OK)
                mt = m * S.out;
        }
        mark[k] = st != COOL_ST_OK;
    }
    for(int q = 0; q < SHQ_COOL_NSTATUS; q++) {
        const unsigned long long b = shq_ballot(st == q);
        if(b && (threadIdx.x & 63) == 0)
            atomicAdd(&s_cnt[q], (unsigned) __popcll((long long) b));
    }
    stat_block_sum(mt, s_w, partial);
    if(threadIdx.x < SHQ_COOL_NSTATUS && s_cnt[threadIdx.x])
        atomicAdd(&cnt[SC_STATUS + threadIdx.x], (unsigned long long) s_cnt[threadIdx.x]);
}

__global__ void stat_positions_kernel(long long m, const int32_t *__restrict__ list, int32_t *pos)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t < m)
        pos[t] = list[pos[t]];
}

/* write_blackhole_txt's loop: column c of the partials is c * nblocks + block */
__global__ __launch_bounds__(256) void stat_bh_totals_kernel(const char *__restrict__ bh, long long nbh, unsigned R, unsigned off_swallowid, unsigned off_mass,
                                                             unsigned off_mdot, unsigned long long *cnt, double *partial)
{
#pragma clang fp contract(off)
    __shared__ double s_w[4];
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    double mass = 0, mdot = 0, medd = 0;
    bool counted = false;
    if(i < nbh) {
        const char *b = bh + (size_t) i * R;
        if(*reinterpret_cast<const unsigned long long *>(b + off_swallowid) == ~0ull) {
            counted = true;
            mass = *reinterpret_cast<const double *>(b + off_mass);
            mdot = *reinterpret_cast<const double *>(b + off_mdot);
            medd = mdot / mass;
        }
    }
    const unsigned long long mk = shq_ballot(counted);
    if(mk && (threadIdx.x & 63) == 0)
        atomicAdd(&cnt[SC_BH_NUM], (unsigned long long) __popcll((long long) mk));
    stat_block_sum(mass, s_w, partial);
    stat_block_sum(mdot, s_w, partial + gridDim.x);
    stat_block_sum(medd, s_w, partial + 2 * (size_t) gridDim.x);
}

constexpr int BHI_WORDS = SHQ_BHINFO_SIZE / 4;
constexpr int BHI_PER_BLOCK = 64; /* records composed per workgroup: 64 * 436 bytes of LDS */

struct BhiWords {
    unsigned *w;
    __device__ void f64(int byte, double x)
    {
        const unsigned long long u = (unsigned long long) __double_as_longlong(x);
        w[byte / 4] = (unsigned) u;
        w[byte / 4 + 1] = (unsigned) (u >> 32);
    }
    __device__ void u64(int byte, unsigned long long u)
    {
        w[byte / 4] = (unsigned) u;
        w[byte / 4 + 1] = (unsigned) (u >> 32);
    }
    __device__ void i32(int byte, int x) { w[byte / 4] = (unsigned) x; }
    __device__ void vec3(int byte, const double *x)
    {
        for(int j = 0; j < 3; j++)
            f64(byte + 8 * j, x[j]);
    }
};

/* collect_BH_info's loop: lane k composes record k of the workgroup's share as words in LDS, then the share is stored word by word */
__global__ __launch_bounds__(BHI_PER_BLOCK) void stat_bh_details_kernel(shq_bh_detail_layout L, shq_bh_detail_arrays X, const char *__restrict__ parts, long long numpart,
                                                                        const char *__restrict__ bh, long long nbh, const int32_t *__restrict__ active,
                                                                        long long nactive, double atime, unsigned *out, unsigned long long *cnt)
{
    __shared__ unsigned s_words[BHI_PER_BLOCK * BHI_WORDS];
    const long long k0 = (long long) blockIdx.x * BHI_PER_BLOCK;
    const int nrec = (int) (nactive - k0 < BHI_PER_BLOCK ? nactive - k0 : BHI_PER_BLOCK);
    for(int t = threadIdx.x; t < nrec * BHI_WORDS; t += BHI_PER_BLOCK) /* info is zeroed first (bhinfo.cpp:72) */
        s_words[t] = 0;
    __syncthreads();
    const int k = threadIdx.x;
    if(k < nrec) {
        bool bad = true;
        const long long p_i = active ? (long long) active[k0 + k] : k0 + k;
        if(p_i >= 0 && p_i < numpart) {
            const char *p = parts + (size_t) p_i * L.part_elsize;
            const long long PI = *reinterpret_cast<const int32_t *>(p + L.off_pi);
            if(*reinterpret_cast<const uint8_t *>(p + L.off_type) == 5 && PI >= 0 && PI < nbh && (!X.SPH_SwallowID || PI < X.n_sph_swallowid)) {
                bad = false;
                const char *b = bh + (size_t) PI * L.bh_elsize;
                auto D = [&](size_t off) { return reinterpret_cast<const double *>(b + off); };
                BhiWords I{s_words + k * BHI_WORDS};
                const int size = SHQ_BHINFO_SIZE - 2 * (int) sizeof(int);
                I.i32(0, size);
                I.i32(432, size);
                I.u64(4, *reinterpret_cast<const unsigned long long *>(p + L.off_id));
                I.f64(12, *D(L.bh_off_mass));
                I.f64(20, *D(L.bh_off_mdot));
                I.f64(28, *D(L.bh_off_density));
                I.i32(36, *reinterpret_cast<const uint8_t *>(b + L.bh_off_mintimebin));
                I.i32(40, *reinterpret_cast<const int8_t *>(b + L.bh_off_encounter));
                if(X.BH_Entropy)
                    I.f64(76, X.BH_Entropy[PI]);
                const double *pos = reinterpret_cast<const double *>(p + L.off_pos);
                for(int j = 0; j < 3; j++) {
                    I.f64(44 + 8 * j, D(L.bh_off_minpotpos)[j] - X.CurrentParticleOffset[j]);
                    I.f64(180 + 8 * j, pos[j] - X.CurrentParticleOffset[j]);
                }
                if(X.BH_SurroundingGasVel)
                    I.vec3(84, X.BH_SurroundingGasVel + 3 * PI);
                if(X.BH_accreted_momentum)
                    I.vec3(108, X.BH_accreted_momentum + 3 * PI);
                I.vec3(276, D(L.bh_off_dragaccel));
                I.vec3(300, reinterpret_cast<const double *>(p + L.off_fulltreegravaccel));
                I.vec3(324, reinterpret_cast<const double *>(p + L.off_vel));
                I.vec3(252, D(L.bh_off_dfaccel));
                I.f64(68, *D(L.bh_off_minpot));
                I.f64(204, *D(L.bh_off_df_surroundingdensity));
                I.f64(244, *D(L.bh_off_df_surroundingrmsvel));
                I.vec3(220, D(L.bh_off_df_surroundingvel));
                if(X.BH_accreted_BHMass)
                    I.f64(140, X.BH_accreted_BHMass[PI]);
                if(X.BH_accreted_Mass)
                    I.f64(132, X.BH_accreted_Mass[PI]);
                if(X.BH_FeedbackWeightSum)
                    I.f64(148, X.BH_FeedbackWeightSum[PI]);
                if(X.SPH_SwallowID)
                    I.u64(156, X.SPH_SwallowID[PI]);
                I.u64(164, *reinterpret_cast<const unsigned long long *>(b + L.bh_off_swallowid));
                I.i32(172, *reinterpret_cast<const int32_t *>(b + L.bh_off_countprogs));
                I.i32(176, (*reinterpret_cast<const uint8_t *>(p + L.off_flags) >> 1) & 1);
                I.f64(348, *D(L.bh_off_mtrack));
                I.f64(356, (double) *reinterpret_cast<const float *>(p + L.off_mass));
                I.f64(364, *D(L.bh_off_kineticfdbkenergy));
                if(X.NumDM)
                    I.f64(372, X.NumDM[PI]);
                I.f64(404, *D(L.bh_off_vdisp));
                if(X.MgasEnc)
                    I.f64(412, X.MgasEnc[PI]);
                if(X.KEflag)
                    I.i32(420, X.KEflag[PI]);
                I.f64(424, atime);
            }
        }
        if(bad)
            cnt[SC_BH_BAD] = 1;
    }
    __syncthreads();
    unsigned *g = out + (size_t) k0 * BHI_WORDS;
    for(int t = threadIdx.x; t < nrec * BHI_WORDS; t += BHI_PER_BLOCK)
        g[t] = s_words[t];
}

inline bool inside(size_t off, size_t size, size_t rec) { return off != SHQ_NOFIELD && off % size == 0 && off + size <= rec; }

int stat_counters_reset(shq_context *ctx)
{
    SHQ_TRY(ctx->stat_cnt.reserve(SC_N));
    SHQ_HIP(hipMemsetAsync(ctx->stat_cnt.ptr, 0, sizeof(unsigned long long) * SC_N, ctx->stream));
    return SHQ_OK;
}

int stat_counters(shq_context *ctx, unsigned long long h[SC_N])
{
    SHQ_HIP(hipMemcpyAsync(h, ctx->stat_cnt.ptr, sizeof(unsigned long long) * SC_N, hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    return SHQ_OK;
}

} // namespace

extern "C" int shq_stats_finish(const shq_stats_sums *summed, shq_stats_state *out)
{
#pragma clang fp contract(off)
    SHQ_CHECK(summed && out, SHQ_ERR_INVALID, "null argument");
    shq_stats_state S;
    memset(&S, 0, sizeof(S));
    int i, j;
    for(i = 0; i < 6; i++) {
        S.MassComp[i] = summed->MassComp[i];
        S.EnergyPotComp[i] = summed->EnergyPotComp[i];
        S.EnergyIntComp[i] = summed->EnergyIntComp[i];
        S.EnergyKinComp[i] = summed->EnergyKinComp[i];
        S.TemperatureComp[i] = summed->TemperatureComp[i];
        for(j = 0; j < 4; j++) {
            S.MomentumComp[i][j] = summed->MomentumComp[i][j];
            S.AngMomentumComp[i][j] = summed->AngMomentumComp[i][j];
            S.CenterOfMassComp[i][j] = summed->CenterOfMassComp[i][j];
        }
    }
    for(i = 0; i < 6; i++)
        S.EnergyTotComp[i] = S.EnergyKinComp[i] + S.EnergyPotComp[i] + S.EnergyIntComp[i];
    S.Mass = S.EnergyKin = S.EnergyPot = S.EnergyInt = S.EnergyTot = 0;
    for(i = 0; i < 6; i++)
        if(S.MassComp[i] > 0)
            S.TemperatureComp[i] /= S.MassComp[i];
    for(j = 0; j < 3; j++)
        S.Momentum[j] = S.AngMomentum[j] = S.CenterOfMass[j] = 0;
    for(i = 0; i < 6; i++) {
        S.Mass += S.MassComp[i];
        S.EnergyKin += S.EnergyKinComp[i];
        S.EnergyPot += S.EnergyPotComp[i];
        S.EnergyInt += S.EnergyIntComp[i];
        S.EnergyTot += S.EnergyTotComp[i];
        for(j = 0; j < 3; j++) {
            S.Momentum[j] += S.MomentumComp[i][j];
            S.AngMomentum[j] += S.AngMomentumComp[i][j];
            S.CenterOfMass[j] += S.CenterOfMassComp[i][j];
        }
    }
    for(i = 0; i < 6; i++)
        for(j = 0; j < 3; j++)
            if(S.MassComp[i] > 0)
                S.CenterOfMassComp[i][j] /= S.MassComp[i];
    for(j = 0; j < 3; j++)
        if(S.Mass > 0)
            S.CenterOfMass[j] /= S.Mass;
    for(i = 0; i < 6; i++) {
        S.CenterOfMassComp[i][3] = S.MomentumComp[i][3] = S.AngMomentumComp[i][3] = 0;
        for(j = 0; j < 3; j++) {
            S.CenterOfMassComp[i][3] += S.CenterOfMassComp[i][j] * S.CenterOfMassComp[i][j];
            S.MomentumComp[i][3] += S.MomentumComp[i][j] * S.MomentumComp[i][j];
            S.AngMomentumComp[i][3] += S.AngMomentumComp[i][j] * S.AngMomentumComp[i][j];
        }
        S.CenterOfMassComp[i][3] = sqrt(S.CenterOfMassComp[i][3]);
        S.MomentumComp[i][3] = sqrt(S.MomentumComp[i][3]);
        S.AngMomentumComp[i][3] = sqrt(S.AngMomentumComp[i][3]);
    }
    S.CenterOfMass[3] = S.Momentum[3] = S.AngMomentum[3] = 0;
    for(j = 0; j < 3; j++) {
        S.CenterOfMass[3] += S.CenterOfMass[j] * S.CenterOfMass[j];
        S.Momentum[3] += S.Momentum[j] * S.Momentum[j];
        S.AngMomentum[3] += S.AngMomentum[j] * S.AngMomentum[j];
    }
    S.CenterOfMass[3] = sqrt(S.CenterOfMass[3]);
    S.Momentum[3] = sqrt(S.Momentum[3]);
    S.AngMomentum[3] = sqrt(S.AngMomentum[3]);
    *out = S;
    return SHQ_OK;
}

extern "C" int shq_energy_statistics(shq_context *ctx, const shq_stats_layout *layout, const void *d_parts, int64_t numpart, const void *d_sph, int64_t nsph,
                                     const shq_stats_params *params, shq_stats_sums *out, int32_t *deferred, int64_t deferred_capacity)
{
    SHQ_CHECK(ctx && layout && params && out && deferred_capacity >= 0 && (deferred || deferred_capacity == 0), SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(numpart >= 0 && numpart < (1ll << 31) - 64 && (d_parts || numpart == 0), SHQ_ERR_INVALID, "energy_statistics: bad particle array");
    const shq_stats_layout &L = *layout;
    const size_t R = L.part_elsize, RS = L.sph_elsize;
    SHQ_CHECK(R >= 8 && R % 8 == 0 && R <= ST_MAXPART && ((uintptr_t) d_parts % 8) == 0, SHQ_ERR_INVALID,
              "energy_statistics: records are 8-byte aligned, a multiple of 8 and at most %zu bytes", ST_MAXPART);
    SHQ_CHECK(inside(L.off_pos, 8, R) && L.off_pos + 24 <= R && inside(L.off_mass, 4, R) && inside(L.off_type, 1, R) && inside(L.off_pi, 4, R) && inside(L.off_vel, 8, R) &&
                  L.off_vel + 24 <= R && inside(L.off_potential, 8, R),
              SHQ_ERR_INVALID, "energy_statistics: Pos, Mass, Type, PI, Vel and Potential must lie aligned inside the particle record");
    SHQ_CHECK(nsph >= 0 && nsph < (1ll << 31) && (d_sph || nsph == 0), SHQ_ERR_INVALID, "energy_statistics: bad gas slot array");
    SHQ_CHECK(RS >= 8 && RS % 8 == 0 && RS <= ST_MAXREC && ((uintptr_t) d_sph % 8) == 0, SHQ_ERR_INVALID,
              "energy_statistics: gas slots are 8-byte aligned, a multiple of 8 and at most %zu bytes", ST_MAXREC);
    SHQ_CHECK(inside(L.sph_off_density, 8, RS) && inside(L.sph_off_entropy, 8, RS) && inside(L.sph_off_ne, 8, RS) &&
                  (L.sph_off_local_j21 == SHQ_NOFIELD || inside(L.sph_off_local_j21, 8, RS)) && (L.sph_off_zreion == SHQ_NOFIELD || inside(L.sph_off_zreion, 8, RS)),
              SHQ_ERR_INVALID, "energy_statistics: Density, Entropy, Ne, local_J21 and zreion must lie aligned inside the gas slot");
    const bool want_t = params->want_temperature != 0;
    if(want_t) {
        SHQ_CHECK(params->uvbg_mode >= SHQ_COOL_UVBG_GLOBAL && params->uvbg_mode <= SHQ_COOL_UVBG_J21, SHQ_ERR_INVALID, "energy_statistics: uvbg_mode = %d",
                  params->uvbg_mode);
        SHQ_CHECK(params->uvbg_mode != SHQ_COOL_UVBG_J21 || (L.sph_off_local_j21 != SHQ_NOFIELD && L.sph_off_zreion != SHQ_NOFIELD), SHQ_ERR_INVALID,
                  "energy_statistics: the J21 mode needs local_J21 and zreion in the gas slot");
        SHQ_CHECK(ctx->cool_have, SHQ_ERR_STATE, "energy_statistics: shq_cooling_set_tables first");
        SHQ_CHECK(params->uvbg_mode != SHQ_COOL_UVBG_ZREION || ctx->cool_znside > 0, SHQ_ERR_STATE, "energy_statistics: the Zreion mode needs a Zreion table");
    }
    shq_stats_sums r;
    memset(&r, 0, sizeof(r));
    if(numpart == 0) {
        *out = r;
        return SHQ_OK;
    }
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SHQ_TRY(stat_counters_reset(ctx));
    unsigned long long *cnt = ctx->stat_cnt.ptr;
    StatArgs A;
    A.L = L;
    A.a1 = params->Time;
    A.a2 = params->Time * params->Time;
    A.a3 = params->Time * params->Time * params->Time;
    A.parts = static_cast<const char *>(d_parts);
    A.sph = static_cast<const char *>(d_sph);
    A.numpart = numpart;
    A.nsph = nsph;
    A.wide = R % 16 == 0 && (uintptr_t) d_parts % 16 == 0;
    A.pitch = (unsigned) st_pitch(R);
    A.nblocks = nblk(numpart, ST_TILE);
    /* the block partials by column, then the 74 sums; the temperature pass has one partial per workgroup of its own behind them */
    const size_t ntblocks = nblk(numpart, 256);
    SHQ_TRY(ctx->stat_part.reserve((size_t) A.nblocks * STAT_NCOL + ntblocks + STAT_NCOL + 1));
    double *partial = ctx->stat_part.ptr, *tpartial = partial + (size_t) A.nblocks * STAT_NCOL, *sums = tpartial + ntblocks;
    if(want_t)
        SHQ_TRY(ctx->stat_mark.reserve((size_t) numpart));
    hipEvent_t eb = ctx->ev_begin[SHQ_T_SPH], ee = ctx->ev_end[SHQ_T_SPH];
    SHQ_HIP(hipEventRecord(eb, st));
    stat_energy_kernel<<<dim3(A.nblocks), dim3(ST_TILE), (size_t) ST_TILE * A.pitch, st>>>(A, want_t ? ctx->stat_mark.ptr : nullptr, cnt, partial);
    SHQ_HIP(hipGetLastError());
    stat_final_sum_kernel<<<dim3(STAT_NCOL), dim3(256), 0, st>>>((long long) A.nblocks, partial, sums);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipEventRecord(ee, st));
    unsigned long long h[SC_N];
    SHQ_TRY(stat_counters(ctx, h));
    SHQ_CHECK(h[SC_BADPI] == 0, SHQ_ERR_INVALID, "energy_statistics: %llu gas particles have their PI outside the slot array", h[SC_BADPI]);
    int64_t ngas = 0, ndef = 0;
    if(want_t && h[SC_COUNT] > 0) {
        SHQ_TRY(ctx->stat_list.reserve((size_t) h[SC_COUNT]));
        SHQ_TRY(shq_marked_list(ctx, ctx->stat_mark.ptr, numpart, ctx->stat_list.ptr, &ngas));
        StatUV U;
        memset(&U, 0, sizeof(U));
        U.ztab = ctx->cool_zreion.ptr;
        U.znside = ctx->cool_znside;
        U.zbox = ctx->cool_zbox;
        U.mode = params->uvbg_mode;
        U.global = shq_cooling_uv(&params->GlobalUVBG);
        for(int d = 0; d < 3; d++)
            U.offset[d] = params->CurrentParticleOffset[d];
        for(int c = 0; c < 6; c++)
            U.j21c[c] = params->J21_coeffs[c];
        U.ss_grey = params->ss_greyopac_factor;
        U.ss_fbar = params->ss_fbar_factor;
        U.redshift = 1. / params->Time - 1;
        const CoolTabs T{ctx->cool_ion.ptr, ctx->cool_rates.ptr, ctx->cool_par.metal_on ? ctx->cool_metal.ptr : nullptr};
        const unsigned nb = nblk(ngas, 256);
        stat_temperature_kernel<<<dim3(nb), dim3(256), 0, st>>>(A, U, ctx->cool_par, T, ctx->stat_list.ptr, (long long) ngas, ctx->stat_mark.ptr, cnt, tpartial);
        SHQ_HIP(hipGetLastError());
        stat_final_sum_kernel<<<dim3(1), dim3(256), 0, st>>>((long long) nb, tpartial, sums + STAT_NCOL);
        SHQ_HIP(hipGetLastError());
        SHQ_HIP(hipEventRecord(ee, st));
        SHQ_TRY(stat_counters(ctx, h));
        if(h[SC_COUNT] != h[SC_STATUS + COOL_ST_OK]) { /* the list positions that did not end OK, then their particle indices, in order */
            SHQ_TRY(ctx->stat_pos.reserve((size_t) ngas));
            int32_t *pos = ctx->stat_pos.ptr;
            SHQ_TRY(shq_marked_list(ctx, ctx->stat_mark.ptr, ngas, pos, &ndef));
            stat_positions_kernel<<<dim3(nblk(ndef)), dim3(256), 0, st>>>((long long) ndef, ctx->stat_list.ptr, pos);
            SHQ_HIP(hipGetLastError());
            const int64_t ncopy = ndef < deferred_capacity ? ndef : deferred_capacity;
            if(ncopy > 0)
                SHQ_HIP(hipMemcpyAsync(deferred, pos, sizeof(int32_t) * (size_t) ncopy, hipMemcpyDeviceToHost, st));
        }
    }
    double hs[STAT_NCOL + 1];
    hs[STAT_NCOL] = 0;
    SHQ_HIP(hipMemcpyAsync(hs, sums, sizeof(double) * (STAT_NCOL + (ngas > 0 ? 1 : 0)), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    float ms = 0;
    SHQ_HIP(hipEventElapsedTime(&ms, eb, ee));
    for(int t = 0; t < 6; t++) {
        const double *c = hs + t * STAT_PER_TYPE;
        r.MassComp[t] = c[0];
        r.EnergyPotComp[t] = c[1];
        r.EnergyKinComp[t] = c[2];
        for(int j = 0; j < 3; j++) {
            r.MomentumComp[t][j] = c[3 + j];
            r.AngMomentumComp[t][j] = c[6 + j];
            r.CenterOfMassComp[t][j] = c[9 + j];
        }
        r.count[t] = (int64_t) h[SC_COUNT + t];
    }
    r.EnergyIntComp[0] = hs[STAT_EINT];
    r.TemperatureComp[0] = hs[STAT_NCOL];
    r.n_bad_type = (int64_t) h[SC_BADTYPE];
    for(int q = 0; q < SHQ_COOL_NSTATUS; q++)
        r.n_status[q] = (int64_t) h[SC_STATUS + q];
    r.n_deferred = ndef;
    r.kernel_ms = ms;
    *out = r;
    SHQ_CHECK(ndef <= deferred_capacity, SHQ_ERR_NOMEM, "energy_statistics: %lld deferred particles, room for %lld", (long long) ndef, (long long) deferred_capacity);
    return SHQ_OK;
}

extern "C" int shq_bh_totals(shq_context *ctx, const void *d_bh, int64_t nbh, size_t bh_elsize, size_t off_swallowid, size_t off_mass, size_t off_mdot, int64_t *num,
                             double sums[3])
{
    SHQ_CHECK(ctx && num && sums, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(nbh >= 0 && nbh < (1ll << 31) && (d_bh || nbh == 0), SHQ_ERR_INVALID, "bh_totals: bad black-hole slot array");
    const size_t R = bh_elsize;
    SHQ_CHECK(R >= 8 && R % 8 == 0 && R <= ST_MAXREC && ((uintptr_t) d_bh % 8) == 0 && inside(off_swallowid, 8, R) && inside(off_mass, 8, R) && inside(off_mdot, 8, R),
              SHQ_ERR_INVALID, "bh_totals: slots are 8-byte aligned, a multiple of 8 and at most %zu bytes, with SwallowID, Mass and Mdot aligned inside", ST_MAXREC);
    *num = 0;
    sums[0] = sums[1] = sums[2] = 0;
    if(nbh == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SHQ_TRY(stat_counters_reset(ctx));
    const unsigned nb = nblk(nbh, 256);
    SHQ_TRY(ctx->stat_part.reserve((size_t) nb * 3 + 3));
    double *partial = ctx->stat_part.ptr, *out = partial + (size_t) nb * 3;
    stat_bh_totals_kernel<<<dim3(nb), dim3(256), 0, st>>>(static_cast<const char *>(d_bh), (long long) nbh, (unsigned) R, (unsigned) off_swallowid, (unsigned) off_mass,
                                                          (unsigned) off_mdot, ctx->stat_cnt.ptr, partial);
    SHQ_HIP(hipGetLastError());
    stat_final_sum_kernel<<<dim3(3), dim3(256), 0, st>>>((long long) nb, partial, out);
    SHQ_HIP(hipGetLastError());
    double hs[3];
    SHQ_HIP(hipMemcpyAsync(hs, out, sizeof(hs), hipMemcpyDeviceToHost, st));
    unsigned long long h[SC_N];
    SHQ_TRY(stat_counters(ctx, h));
    *num = (int64_t) h[SC_BH_NUM];
    for(int c = 0; c < 3; c++)
        sums[c] = hs[c];
    return SHQ_OK;
}

extern "C" int shq_bh_details(shq_context *ctx, const shq_bh_detail_layout *layout, const void *d_parts, int64_t numpart, const void *d_bh, int64_t nbh,
                              const shq_bh_detail_arrays *arrays, const int32_t *d_active, int64_t nactive, double atime, void *d_out)
{
    SHQ_CHECK(ctx && layout && arrays && nactive >= 0 && (d_out || nactive == 0), SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(numpart >= 0 && numpart < (1ll << 31) && (d_parts || numpart == 0) && nbh >= 0 && nbh < (1ll << 31) && (d_bh || nbh == 0) && nactive < (1ll << 31),
              SHQ_ERR_INVALID, "bh_details: bad array");
    const shq_bh_detail_layout &L = *layout;
    const size_t R = L.part_elsize, RB = L.bh_elsize;
    SHQ_CHECK(R >= 8 && R % 8 == 0 && R <= ST_MAXREC && ((uintptr_t) d_parts % 8) == 0 && RB >= 8 && RB % 8 == 0 && RB <= ST_MAXREC && ((uintptr_t) d_bh % 8) == 0 &&
                  ((uintptr_t) d_out % 4) == 0,
              SHQ_ERR_INVALID, "bh_details: records and slots are 8-byte aligned, a multiple of 8 and at most %zu bytes; the output is 4-byte aligned", ST_MAXREC);
    auto vec = [](size_t off, size_t rec) { return inside(off, 8, rec) && off + 24 <= rec; };
    SHQ_CHECK(vec(L.off_pos, R) && inside(L.off_mass, 4, R) && inside(L.off_flags, 1, R) && inside(L.off_type, 1, R) && inside(L.off_pi, 4, R) && vec(L.off_vel, R) &&
                  vec(L.off_fulltreegravaccel, R) && inside(L.off_id, 8, R),
              SHQ_ERR_INVALID, "bh_details: a member of the particle record lies outside it or is misaligned");
    SHQ_CHECK(inside(L.bh_off_mintimebin, 1, RB) && inside(L.bh_off_encounter, 1, RB) && inside(L.bh_off_mass, 8, RB) && inside(L.bh_off_mdot, 8, RB) &&
                  inside(L.bh_off_density, 8, RB) && inside(L.bh_off_mtrack, 8, RB) && inside(L.bh_off_kineticfdbkenergy, 8, RB) && inside(L.bh_off_vdisp, 8, RB) &&
                  vec(L.bh_off_dfaccel, RB) && vec(L.bh_off_df_surroundingvel, RB) && inside(L.bh_off_df_surroundingrmsvel, 8, RB) &&
                  inside(L.bh_off_df_surroundingdensity, 8, RB) && vec(L.bh_off_dragaccel, RB) && inside(L.bh_off_swallowid, 8, RB) && inside(L.bh_off_minpot, 8, RB) &&
                  vec(L.bh_off_minpotpos, RB) && inside(L.bh_off_countprogs, 4, RB),
              SHQ_ERR_INVALID, "bh_details: a member of the black-hole slot lies outside it or is misaligned");
    SHQ_CHECK(!arrays->SPH_SwallowID || arrays->n_sph_swallowid >= 0, SHQ_ERR_INVALID, "bh_details: n_sph_swallowid = %lld", (long long) arrays->n_sph_swallowid);
    if(nactive == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(stat_counters_reset(ctx));
    stat_bh_details_kernel<<<dim3(nblk(nactive, BHI_PER_BLOCK)), dim3(BHI_PER_BLOCK), 0, ctx->stream>>>(
        L, *arrays, static_cast<const char *>(d_parts), (long long) numpart, static_cast<const char *>(d_bh), (long long) nbh, d_active, (long long) nactive, atime,
        static_cast<unsigned *>(d_out), ctx->stat_cnt.ptr);
    SHQ_HIP(hipGetLastError());
    unsigned long long h[SC_N];
    SHQ_TRY(stat_counters(ctx, h));
    SHQ_CHECK(h[SC_BH_BAD] == 0, SHQ_ERR_INVALID,
              "bh_details: an active index outside the particles, a supposed black hole of another type, or a PI outside its arrays");
    return SHQ_OK;
}
