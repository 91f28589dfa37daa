/* startup.hip — what the reference does between petaio_read_snapshot and the first step (include/shenqi_hip.h, "Run start-up").
 *
 *   check_omega / check_positions / check_smoothing_length / init()'s loop   init.cpp:203-214, 313-335, 342-359, 119-188   shq_startup_particles
 *   check_density_entropy                                                    init.cpp:363-388                              shq_startup_check_density_entropy
 *   set_init_hsml                                                            density2.cpp:164-203                          shq_set_init_hsml
 *   the entropy of setup_smoothinglengths / setup_density_indep_entropy      init.cpp:422-423, 518                         shq_init_entropy
 *   setup_smoothinglengths                                                   init.cpp:402-521                              shq_setup_smoothinglengths
 *
 * The record pass (the tile copies are in record_tile.hpp).  A workgroup of ST_TILE threads owns ST_TILE consecutive particle records.  It copies them into LDS with 16-byte
 * loads, consecutive lanes on consecutive pieces (the records are contiguous, so this is a stream), ST_BATCH loads in flight per lane
 * as in snapshot.hip's gather; lane k then runs every selected loop on record k in LDS, and if a loop changed a member the tile is
 * streamed back the same way.  The LDS row pitch is the record size rounded up to an odd number of 8-byte words (160 -> 168), as in
 * snapshot.hip.  The gas and black-hole slots are written by the lane that owns the particle.
 * The mass sums: a butterfly over the wave (the same shape for every wave), the four wave sums added in wave order, one partial per
 * workgroup; a second kernel adds the partials in a fixed order.  No floating-point atomics, so equal inputs give equal bytes. */
#include "common.hpp"
#include "record_tile.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int ST_MAXCLIMB = 64; /* a father chain longer than this is no tree (the deepest cell is Box / 2^21 wide) */
/* GAMMA_MINUS1 as the reference forms it (physconst.h:35-36) */
#define ST_GAMMA_MINUS1 ((5.0 / 3.0) - 1)
#define ST_HYDROGEN_MASSFRAC 0.76 /* physconst.h:38 */
/* st_cnt: counters and indices */
enum { C_BADMASS = 0, C_NOUTSIDE, C_NUMZERO, C_NUMPROB, C_NBADDELAY, C_FIRST_OUTSIDE, C_LASTZERO, C_LASTPROB, C_FIRST_BADDELAY, C_BADPI, C_BADMOM, C_BADHSML,
       C_BADCHAIN, C_BADDENS, C_MAXDIFF, C_N };
constexpr unsigned long long ST_NONE = ~0ull;

__global__ void st_reset_kernel(unsigned long long *cnt)
{
    const int k = threadIdx.x;
    if(k < C_N)
        cnt[k] = (k == C_FIRST_OUTSIDE || k == C_FIRST_BADDELAY) ? ST_NONE : 0ull; /* the two "highest index" cells hold index + 1 */
}

__device__ __forceinline__ double st_pick6(const double a[6], int t)
{
    double v = a[0];
#pragma unroll
    for(int k = 1; k < 6; k++)
        v = t == k ? a[k] : v;
    return v;
}

/* count, lowest and highest lane of a wave-wide condition into the workgroup's cells: one LDS atomic per wave and cell */
__device__ __forceinline__ void st_tally(bool p, int first_index_of_wave, unsigned *cnt, int *lowest, int *highest)
{
    const unsigned long long m = shq_ballot(p);
    if(m == 0 || (threadIdx.x & 63) != 0)
        return;
    atomicAdd(cnt, (unsigned) __popcll((long long) m));
    if(lowest)
        atomicMin(lowest, first_index_of_wave + (__ffsll((long long) m) - 1));
    if(highest)
        atomicMax(highest, first_index_of_wave + (63 - __clzll((long long) m)));
}

/* before init()'s loop writes anything: the slot of every gas and black-hole particle lies inside its array */
__global__ void st_check_pi_kernel(const char *__restrict__ parts, long long numpart, unsigned R, unsigned off_type, unsigned off_pi, long long nsph, long long nbh,
                                   unsigned long long *cnt)
{
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= numpart)
        return;
    const char *p = parts + (size_t) i * R;
    const int type = *reinterpret_cast<const uint8_t *>(p + off_type);
    if(type != 0 && type != 5)
        return;
    const long long pi = *reinterpret_cast<const int32_t *>(p + off_pi);
    if(pi < 0 || pi >= (type == 0 ? nsph : nbh))
        cnt[C_BADPI] = 1;
}

__global__ __launch_bounds__(ST_TILE) void st_particles_kernel(shq_startup_layout L, shq_startup_params P, char *parts, long long numpart, char *sph, long long nsph, char *bh,
                                                              long long nbh, int which, int wide, unsigned pitch, unsigned long long *cnt, double *partial)
{
#pragma clang fp contract(off)
    extern __shared__ uint2 st_tile_[];
    __shared__ double s_wsum[ST_TILE / 64][7];
    __shared__ unsigned s_cnt[5];
    __shared__ int s_low[2], s_high[2], s_dirty;
    char *lds = reinterpret_cast<char *>(st_tile_);
    const int k = threadIdx.x;
    const long long row0 = (long long) blockIdx.x * ST_TILE;
    const int nrow = (int) (numpart - row0 < ST_TILE ? numpart - row0 : ST_TILE);
    if(k < 5)
        s_cnt[k] = 0;
    if(k < 2) {
        s_low[k] = 0x7fffffff;
        s_high[k] = -1;
    }
    if(k == 0)
        s_dirty = 0;
    char *gtile = parts + (size_t) row0 * L.part_elsize;
    if(wide)
        st_stage_in<16>(lds, pitch, gtile, (unsigned) L.part_elsize, nrow);
    else
        st_stage_in<8>(lds, pitch, gtile, (unsigned) L.part_elsize, nrow);
    __syncthreads();
    const bool live = k < nrow;
    char *rec = lds + (unsigned) (live ? k : 0) * pitch;
    const int type = live ? *reinterpret_cast<const uint8_t *>(rec + L.off_type) : -1;
    bool dirty = false;
    bool f_badmass = false, f_outside = false, f_zero = false, f_prob = false, f_delay = false;
    double m = 0;
    if(live && (which & (SHQ_STARTUP_OMEGA | SHQ_STARTUP_INIT))) {
        float mass = *reinterpret_cast<const float *>(rec + L.off_mass);
        if(which & SHQ_STARTUP_OMEGA) {
            if(mass == 0) { /* zeros written to the saved mass array: recover the true mass */
                f_badmass = true;
                if(type < 6) {
                    const int gen = *reinterpret_cast<const uint8_t *>(rec + L.off_flags) >> 4;
                    mass = (float) (st_pick6(P.MassTable, type) * (1. - (double) gen / P.generations));
                    *reinterpret_cast<float *>(rec + L.off_mass) = mass;
                    dirty = true;
                }
            }
            m = mass;
        }
    }
    if(live && (which & SHQ_STARTUP_POSITIONS)) {
        const double *pos = reinterpret_cast<const double *>(rec + L.off_pos);
        for(int j = 0; j < 3; j++)
            if(pos[j] < 0 || pos[j] > P.BoxSize || !isfinite(pos[j]))
                f_outside = true;
        f_zero = pos[0] < 1e-35 && pos[1] < 1e-35 && pos[2] < 1e-35;
    }
    if(live && (which & SHQ_STARTUP_HSML) && (type == 0 || type == 5)) {
        double *h = reinterpret_cast<double *>(rec + L.off_hsml);
        if(*h > P.BoxSize || *h <= 0) {
            *h = st_pick6(P.MeanSeparation, type);
            f_prob = true;
            dirty = true;
        }
    }
    if(live && (which & SHQ_STARTUP_INIT)) {
        *reinterpret_cast<long long *>(rec + L.off_ti_drift) = (long long) P.Ti_Current;
        dirty = true;
        const long long pi = *reinterpret_cast<const int32_t *>(rec + L.off_pi);
        if(type == 4) { /* zero star smoothing lengths are not saved in the snapshots */
            double *h = reinterpret_cast<double *>(rec + L.off_hsml);
            if(*h == 0)
                *h = 0.1 * P.MeanSeparation[0];
        }
        if(type == 5 && pi >= 0 && pi < nbh) { /* the range has been checked; the test keeps a broken caller inside the array */
            char *b = bh + (size_t) pi * L.bh_elsize;
            if(P.RestartSnapNum == -1)
                *reinterpret_cast<double *>(b + L.bh_off_mass) = (double) *reinterpret_cast<const float *>(rec + L.off_mass);
            for(int j = 0; j < 3; j++) {
                reinterpret_cast<double *>(b + L.bh_off_dfaccel)[j] = 0;
                reinterpret_cast<double *>(b + L.bh_off_dragaccel)[j] = 0;
            }
        }
        if(type == 0 && pi >= 0 && pi < nsph) {
            char *s = sph + (size_t) pi * L.sph_elsize;
            for(int j = 0; j < 3; j++)
                reinterpret_cast<double *>(s + L.sph_off_hydroaccel)[j] = 0;
            if(!isfinite(*reinterpret_cast<const double *>(s + L.sph_off_delaytime)))
                f_delay = true;
            *reinterpret_cast<double *>(s + L.sph_off_dtentropy) = 0;
            if(P.RestartSnapNum == -1) {
                *reinterpret_cast<double *>(s + L.sph_off_density) = -1;
                *reinterpret_cast<double *>(s + L.sph_off_egywtdensity) = -1;
                *reinterpret_cast<double *>(s + L.sph_off_dhsmlegydensityfactor) = -1;
                *reinterpret_cast<double *>(s + L.sph_off_entropy) = -1;
                *reinterpret_cast<double *>(s + L.sph_off_ne) = 1.0;
                *reinterpret_cast<double *>(s + L.sph_off_divvel) = 0;
                *reinterpret_cast<double *>(s + L.sph_off_curlvel) = 0;
                *reinterpret_cast<double *>(s + L.sph_off_delaytime) = 0;
                *reinterpret_cast<double *>(s + L.sph_off_metallicity) = 0;
                float *metals = reinterpret_cast<float *>(s + L.sph_off_metals);
                for(unsigned j = 0; j < (unsigned) L.sph_nmetals; j++)
                    metals[j] = 0;
                if(L.sph_nmetals > 0)
                    metals[0] = ST_HYDROGEN_MASSFRAC; /* primordial abundances of H and He */
                if(L.sph_nmetals > 1)
                    metals[1] = 1 - ST_HYDROGEN_MASSFRAC;
                *reinterpret_cast<double *>(s + L.sph_off_sfr) = 0;
                *reinterpret_cast<double *>(s + L.sph_off_maxsignalvel) = 0;
            }
            if(P.init_reion && L.sph_off_local_j21 != SHQ_NOFIELD && L.sph_off_zreion != SHQ_NOFIELD) {
                *reinterpret_cast<double *>(s + L.sph_off_local_j21) = 0;
                *reinterpret_cast<double *>(s + L.sph_off_zreion) = -1;
            }
        }
    }
    if(dirty)
        s_dirty = 1;
    const int wbase = (int) (row0 + (k & ~63)); /* numpart < 2^31 - 64 */
    if(which & SHQ_STARTUP_OMEGA)
        st_tally(f_badmass, wbase, &s_cnt[0], nullptr, nullptr);
    if(which & SHQ_STARTUP_POSITIONS) {
        st_tally(f_outside, wbase, &s_cnt[1], &s_low[0], nullptr);
        st_tally(f_zero, wbase, &s_cnt[2], nullptr, &s_high[0]);
    }
    if(which & SHQ_STARTUP_HSML)
        st_tally(f_prob, wbase, &s_cnt[3], nullptr, &s_high[1]);
    if(which & SHQ_STARTUP_INIT)
        st_tally(f_delay, wbase, &s_cnt[4], &s_low[1], nullptr);
    if(which & SHQ_STARTUP_OMEGA) { /* the six sums by type and the total: the same butterfly in every wave */
        double v[7];
#pragma unroll
        for(int t = 0; t < 6; t++)
            v[t] = type == t ? m : 0.0;
        v[6] = m;
#pragma unroll
        for(int off = 32; off >= 1; off >>= 1)
#pragma unroll
            for(int t = 0; t < 7; t++)
                v[t] += __shfl_xor(v[t], off, 64);
        if((k & 63) == 0)
#pragma unroll
            for(int t = 0; t < 7; t++)
                s_wsum[k >> 6][t] = v[t];
    }
    __syncthreads();
    if((which & SHQ_STARTUP_OMEGA) && k < 7) {
        double s = s_wsum[0][k];
        for(int w = 1; w < ST_TILE / 64; w++)
            s += s_wsum[w][k];
        partial[(size_t) blockIdx.x * 7 + k] = s;
    }
    if(k < 5 && s_cnt[k])
        atomicAdd(&cnt[C_BADMASS + k], (unsigned long long) s_cnt[k]);
    if(k == 5 && s_low[0] != 0x7fffffff)
        atomicMin(&cnt[C_FIRST_OUTSIDE], (unsigned long long) s_low[0]);
    if(k == 6 && s_high[0] >= 0)
        atomicMax(&cnt[C_LASTZERO], (unsigned long long) s_high[0] + 1ull);
    if(k == 7 && s_high[1] >= 0)
        atomicMax(&cnt[C_LASTPROB], (unsigned long long) s_high[1] + 1ull);
    if(k == 8 && s_low[1] != 0x7fffffff)
        atomicMin(&cnt[C_FIRST_BADDELAY], (unsigned long long) s_low[1]);
    if(s_dirty) { /* uniform: read after the barrier */
        if(wide)
            st_stage_out<16>(lds, pitch, gtile, (unsigned) L.part_elsize, nrow);
        else
            st_stage_out<8>(lds, pitch, gtile, (unsigned) L.part_elsize, nrow);
    }
}

/* the block partials in a fixed order: thread j adds partials j, j + 256, ... , then a halving tree over the threads */
__global__ __launch_bounds__(256) void st_final_sum_kernel(long long nblocks, const double *__restrict__ partial, double *out)
{
#pragma clang fp contract(off)
    __shared__ double s[256];
    for(int c = 0; c < 7; c++) {
        double a = 0;
        for(long long b = threadIdx.x; b < nblocks; b += 256)
            a += partial[(size_t) b * 7 + c];
        s[threadIdx.x] = a;
        __syncthreads();
        for(int h = 128; h >= 1; h >>= 1) {
            if((int) threadIdx.x < h)
                s[threadIdx.x] += s[threadIdx.x + h];
            __syncthreads();
        }
        if(threadIdx.x == 0)
            out[c] = s[0];
        __syncthreads();
    }
}

__global__ void st_density_entropy_kernel(shq_startup_layout L, char *sph, long long nsph, double meanbar, double MinEgySpec, double a3, unsigned long long *cnt)
{
#pragma clang fp contract(off)
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if(i < nsph) {
        char *s = sph + (size_t) i * L.sph_elsize;
        double *Density = reinterpret_cast<double *>(s + L.sph_off_density), *Egy = reinterpret_cast<double *>(s + L.sph_off_egywtdensity);
        double *Entropy = reinterpret_cast<double *>(s + L.sph_off_entropy);
        double rho = *Density;
        if(rho <= 0 || !isfinite(rho)) { /* density() will fix this up */
            rho = meanbar;
            *Density = rho;
            bad = true;
        }
        const double e = *Egy;
        if(e <= 0 || !isfinite(e))
            *Egy = rho;
        const double minent = ST_GAMMA_MINUS1 * MinEgySpec / pow(rho / a3, ST_GAMMA_MINUS1);
        if(*Entropy < minent)
            *Entropy = minent;
    }
    const unsigned long long mk = shq_ballot(bad);
    if(mk && (threadIdx.x & 63) == 0)
        atomicAdd(&cnt[C_BADDENS], (unsigned long long) __popcll((long long) mk));
}

/* set_init_hsml's loop.  Particles in index order share ancestors, so the loads of the chain coalesce. */
__global__ __launch_bounds__(256) void st_init_hsml_kernel(long long n, const double4 *__restrict__ posm, const uint8_t *__restrict__ pflags,
                                                           const int32_t *__restrict__ pfather, const int32_t *__restrict__ nfather, const NodeA *__restrict__ A,
                                                           const NodeB *__restrict__ B, long long numnodes, double MeanGasSeparation, double DesNumNgb, double Box,
                                                           double *hsml, int32_t *node_out, const int32_t *__restrict__ order, long long firstnode,
                                                           unsigned long long *cnt)
{
#pragma clang fp contract(off)
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    const unsigned f = pflags[i];
    const int type = (int) (f >> 4);
    if((type != 0 && type != 5) || (f & 1u)) { /* only SPH-like particles; no garbage */
        if(node_out)
            node_out[i] = -1;
        return;
    }
    const double mass = posm[i].w;
    long long no = -1; /* -1: the particle itself */
    long long p = pfather[i];
    bool badchain = false;
    for(int steps = 0;; steps++) {
        if(p < 0 || p >= numnodes) { /* below firstnode: a particle the tree skipped, or the root's father */
            badchain = badchain || p >= numnodes;
            break;
        }
        no = p;
        if(!(10 * DesNumNgb * mass > A[no].mass))
            break;
        if(steps >= ST_MAXCLIMB) {
            badchain = true;
            break;
        }
        p = nfather[no];
    }
    double h = MeanGasSeparation;
    bool badmom = false;
    if(no >= 0) {
        const double len = B[no].len, nodemass = A[no].mass;
        badmom = len > Box || nodemass < mass;
        const double testhsml = len * pow(3.0 / (4 * M_PI) * DesNumNgb * mass / nodemass, 1.0 / 3);
        if(testhsml < 500. * MeanGasSeparation) /* recover from a poor initial guess */
            h = testhsml;
    }
    hsml[i] = h;
    if(node_out)
        node_out[i] = no >= 0 ? (int32_t) (firstnode + (order ? (long long) order[no] : no)) : (int32_t) i;
    if(badmom)
        atomicAdd(&cnt[C_BADMOM], 1ull);
    if(h <= 0)
        atomicAdd(&cnt[C_BADHSML], 1ull);
    if(badchain)
        atomicAdd(&cnt[C_BADCHAIN], 1ull);
}

__global__ void st_entropy_kernel(long long n, const uint8_t *__restrict__ pflags, const double *__restrict__ X, double *entropy, double *old, double u_init, double a3)
{
#pragma clang fp contract(off)
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n || (pflags[i] >> 4) != 0)
        return;
    const double x = X[i];
    entropy[i] = ST_GAMMA_MINUS1 * u_init / pow(x / a3, ST_GAMMA_MINUS1);
    if(old)
        old[i] = x;
}

/* max over gas of |EgyWtDensity - old| / EgyWtDensity: a maximum does not depend on the order, and non-negative doubles order as their
 * bit patterns do */
__global__ void st_maxdiff_kernel(long long n, const uint8_t *__restrict__ pflags, const double *__restrict__ egy, const double *__restrict__ old,
                                  unsigned long long *cnt)
{
#pragma clang fp contract(off)
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    double v = 0;
    if(i < n && (pflags[i] >> 4) == 0) {
        const double value = fabs(egy[i] - old[i]) / egy[i];
        if(value > v)
            v = value;
    }
    for(int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    if((threadIdx.x & 63) == 0 && v > 0)
        atomicMax(&cnt[C_MAXDIFF], (unsigned long long) __double_as_longlong(v));
}

inline bool inside(size_t off, size_t size, size_t rec) { return off != SHQ_NOFIELD && off % size == 0 && off + size <= rec; }

int check_part_layout(const shq_startup_layout *l, const void *d_parts, int64_t numpart)
{
    SHQ_CHECK(l && numpart >= 0 && numpart < (1ll << 31) - 64 && (d_parts || numpart == 0), SHQ_ERR_INVALID, "startup: bad particle array");
    const size_t R = l->part_elsize;
    SHQ_CHECK(R >= 8 && R % 8 == 0 && R <= ST_MAXPART && ((uintptr_t) d_parts % 8) == 0, SHQ_ERR_INVALID,
              "startup: records are 8-byte aligned, a multiple of 8 and at most %zu bytes", ST_MAXPART);
    SHQ_CHECK(inside(l->off_pos, 8, R) && l->off_pos + 24 <= R && inside(l->off_mass, 4, R) && inside(l->off_flags, 1, R) && inside(l->off_type, 1, R) &&
                  inside(l->off_pi, 4, R) && inside(l->off_hsml, 8, R) && inside(l->off_ti_drift, 8, R),
              SHQ_ERR_INVALID, "startup: Pos, Mass, the flag byte, Type, PI, Hsml and Ti_drift must lie aligned inside the particle record");
    return SHQ_OK;
}

int check_sph_layout(const shq_startup_layout *l, const void *d_sph, int64_t nsph, bool all_members)
{
    SHQ_CHECK(nsph >= 0 && nsph < (1ll << 31) && (d_sph || nsph == 0), SHQ_ERR_INVALID, "startup: bad gas slot array");
    const size_t R = l->sph_elsize;
    SHQ_CHECK(R >= 8 && R % 8 == 0 && R <= ST_MAXREC && ((uintptr_t) d_sph % 8) == 0, SHQ_ERR_INVALID,
              "startup: gas slots are 8-byte aligned, a multiple of 8 and at most %zu bytes", ST_MAXREC);
    SHQ_CHECK(inside(l->sph_off_density, 8, R) && inside(l->sph_off_egywtdensity, 8, R) && inside(l->sph_off_entropy, 8, R), SHQ_ERR_INVALID,
              "startup: Density, EgyWtDensity and Entropy must lie aligned inside the gas slot");
    if(!all_members)
        return SHQ_OK;
    SHQ_CHECK(inside(l->sph_off_dtentropy, 8, R) && inside(l->sph_off_maxsignalvel, 8, R) && inside(l->sph_off_hydroaccel, 8, R) && l->sph_off_hydroaccel + 24 <= R &&
                  inside(l->sph_off_dhsmlegydensityfactor, 8, R) && inside(l->sph_off_divvel, 8, R) && inside(l->sph_off_curlvel, 8, R) && inside(l->sph_off_sfr, 8, R) &&
                  inside(l->sph_off_ne, 8, R) && inside(l->sph_off_delaytime, 8, R) && inside(l->sph_off_metallicity, 8, R),
              SHQ_ERR_INVALID, "startup: a member of the gas slot lies outside it or is misaligned");
    SHQ_CHECK(l->sph_nmetals <= 64 && (l->sph_nmetals == 0 || (inside(l->sph_off_metals, 4, R) && l->sph_off_metals + 4 * l->sph_nmetals <= R)), SHQ_ERR_INVALID,
              "startup: Metals[%zu] leaves the gas slot", l->sph_nmetals);
    SHQ_CHECK((l->sph_off_local_j21 == SHQ_NOFIELD || inside(l->sph_off_local_j21, 8, R)) && (l->sph_off_zreion == SHQ_NOFIELD || inside(l->sph_off_zreion, 8, R)),
              SHQ_ERR_INVALID, "startup: local_J21 / zreion lie outside the gas slot or are misaligned");
    return SHQ_OK;
}

int check_bh_layout(const shq_startup_layout *l, const void *d_bh, int64_t nbh)
{
    SHQ_CHECK(nbh >= 0 && nbh < (1ll << 31) && (d_bh || nbh == 0), SHQ_ERR_INVALID, "startup: bad black-hole slot array");
    const size_t R = l->bh_elsize;
    SHQ_CHECK(R >= 8 && R % 8 == 0 && R <= ST_MAXREC && ((uintptr_t) d_bh % 8) == 0, SHQ_ERR_INVALID,
              "startup: black-hole slots are 8-byte aligned, a multiple of 8 and at most %zu bytes", ST_MAXREC);
    SHQ_CHECK(inside(l->bh_off_mass, 8, R) && inside(l->bh_off_dfaccel, 8, R) && l->bh_off_dfaccel + 24 <= R && inside(l->bh_off_dragaccel, 8, R) &&
                  l->bh_off_dragaccel + 24 <= R,
              SHQ_ERR_INVALID, "startup: Mass, DFAccel and DragAccel must lie aligned inside the black-hole slot");
    return SHQ_OK;
}

int st_reset(shq_context *ctx)
{
    SHQ_TRY(ctx->st_cnt.reserve(C_N));
    st_reset_kernel<<<dim3(1), dim3(64), 0, ctx->stream>>>(reinterpret_cast<unsigned long long *>(ctx->st_cnt.ptr));
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

int st_counters(shq_context *ctx, unsigned long long h[C_N])
{
    SHQ_HIP(hipMemcpyAsync(h, ctx->st_cnt.ptr, sizeof(unsigned long long) * C_N, hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    return SHQ_OK;
}

template <typename T> inline T *hfield(const shq_part_view *v, int64_t i, size_t off)
{
    return reinterpret_cast<T *>(static_cast<char *>(v->base) + (size_t) i * v->elsize + off);
}

} // namespace

extern "C" int shq_startup_mean_separation(double MeanSeparation[6], double BoxSize, const int64_t NTotalInit[6])
{
    SHQ_CHECK(MeanSeparation && NTotalInit, SHQ_ERR_INVALID, "null argument");
    for(int i = 0; i < 6; i++)
        if(NTotalInit[i] > 0)
            MeanSeparation[i] = BoxSize / pow(NTotalInit[i], 1.0 / 3);
    return SHQ_OK;
}

extern "C" int shq_startup_u_init(double InitGasTemp, double CMBTemperature, double atime, double uu_in_cgs, double MinEgySpec, double *u_init_out, double *InitGasTemp_used)
{
#pragma clang fp contract(off)
    SHQ_CHECK(u_init_out, SHQ_ERR_INVALID, "null argument");
    const double BOLTZMANN = 1.38066e-16, PROTONMASS = 1.6726e-24; /* physconst.h:11, 22 */
    if(InitGasTemp < 0)
        InitGasTemp = CMBTemperature / atime;
    double u_init = (1.0 / ST_GAMMA_MINUS1) * (BOLTZMANN / PROTONMASS) * InitGasTemp;
    u_init /= uu_in_cgs; /* unit conversion */
    double molecular_weight;
    if(InitGasTemp > 1.0e4) /* assuming full ionisation */
        molecular_weight = 4 / (8 - 5 * (1 - ST_HYDROGEN_MASSFRAC));
    else /* assuming neutral gas */
        molecular_weight = 4 / (1 + 3 * ST_HYDROGEN_MASSFRAC);
    u_init /= molecular_weight;
    if(u_init < MinEgySpec)
        u_init = MinEgySpec;
    *u_init_out = u_init;
    if(InitGasTemp_used)
        *InitGasTemp_used = InitGasTemp;
    return SHQ_OK;
}

extern "C" int shq_startup_omega(const double mass_type[6], double mass_total, double BoxSize, double RhoCrit, double OmegaNu, int MassiveNuLinRespOn, double Omega0,
                                 double omegas[6], double *omega_out, int *bad)
{
#pragma clang fp contract(off)
    SHQ_CHECK(mass_type && omegas && omega_out && bad, SHQ_ERR_INVALID, "null argument");
    const double massnorm = (BoxSize * BoxSize * BoxSize) * RhoCrit;
    double omega = mass_total / massnorm;
    for(int i = 0; i < 6; i++)
        omegas[i] = mass_type[i] / massnorm;
    if(MassiveNuLinRespOn) /* the density of the analytically followed massive neutrinos */
        omega += OmegaNu;
    *omega_out = omega;
    *bad = fabs(omega - Omega0) > 1.0e-3;
    return SHQ_OK;
}

extern "C" int shq_startup_meanbar(double OmegaBaryon, double HubbleParam, double *meanbar)
{
#pragma clang fp contract(off)
    SHQ_CHECK(meanbar, SHQ_ERR_INVALID, "null argument");
    const double HUBBLE = 3.2407789e-18, GRAVITY = 6.672e-8; /* physconst.h:26, 5 */
    *meanbar = OmegaBaryon * 3 * HUBBLE * HubbleParam * HUBBLE * HubbleParam / (8 * M_PI * GRAVITY);
    return SHQ_OK;
}

extern "C" int shq_startup_particles(shq_context *ctx, const shq_startup_layout *layout, void *d_parts, int64_t numpart, void *d_sph, int64_t nsph, void *d_bh,
                                     int64_t nbh, const shq_startup_params *params, int which, shq_startup_report *report)
{
    SHQ_CHECK(ctx && params && report, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(which > 0 && which < 16, SHQ_ERR_INVALID, "startup_particles: which = %d", which);
    SHQ_TRY(check_part_layout(layout, d_parts, numpart));
    if(which & SHQ_STARTUP_INIT) {
        SHQ_TRY(check_sph_layout(layout, d_sph, nsph, true));
        SHQ_TRY(check_bh_layout(layout, d_bh, nbh));
    }
    memset(report, 0, sizeof(*report));
    report->first_outside = report->lastzero = report->lastprob = report->first_bad_delaytime = -1;
    if(numpart == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SHQ_TRY(st_reset(ctx));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(ctx->st_cnt.ptr);
    unsigned long long h[C_N];
    if(which & SHQ_STARTUP_INIT) {
        st_check_pi_kernel<<<dim3(nblk(numpart)), dim3(256), 0, st>>>((const char *) d_parts, (long long) numpart, (unsigned) layout->part_elsize,
                                                                      (unsigned) layout->off_type, (unsigned) layout->off_pi, (long long) nsph, (long long) nbh, cnt);
        SHQ_HIP(hipGetLastError());
        SHQ_TRY(st_counters(ctx, h));
        SHQ_CHECK(h[C_BADPI] == 0, SHQ_ERR_INVALID, "startup_particles: a gas or black-hole particle has its PI outside the slot array");
    }
    const unsigned nblocks = nblk(numpart, ST_TILE);
    SHQ_TRY(ctx->st_part.reserve((size_t) nblocks * 7 + 8));
    const unsigned pitch = (unsigned) st_pitch(layout->part_elsize);
    const int wide = layout->part_elsize % 16 == 0 && (uintptr_t) d_parts % 16 == 0;
    st_particles_kernel<<<dim3(nblocks), dim3(ST_TILE), (size_t) ST_TILE * pitch, st>>>(*layout, *params, (char *) d_parts, (long long) numpart, (char *) d_sph,
                                                                                       (long long) nsph, (char *) d_bh, (long long) nbh, which, wide, pitch, cnt,
                                                                                       ctx->st_part.ptr);
    SHQ_HIP(hipGetLastError());
    double sums[7] = {0, 0, 0, 0, 0, 0, 0};
    if(which & SHQ_STARTUP_OMEGA) {
        double *out = ctx->st_part.ptr + (size_t) nblocks * 7;
        st_final_sum_kernel<<<dim3(1), dim3(256), 0, st>>>((long long) nblocks, ctx->st_part.ptr, out);
        SHQ_HIP(hipGetLastError());
        SHQ_HIP(hipMemcpyAsync(sums, out, sizeof(sums), hipMemcpyDeviceToHost, st));
    }
    SHQ_TRY(st_counters(ctx, h));
    for(int t = 0; t < 6; t++)
        report->mass_type[t] = sums[t];
    report->mass_total = sums[6];
    report->badmass = (int64_t) h[C_BADMASS];
    report->noutside = (int64_t) h[C_NOUTSIDE];
    report->first_outside = h[C_FIRST_OUTSIDE] == ST_NONE ? -1 : (int64_t) h[C_FIRST_OUTSIDE];
    report->numzero = (int64_t) h[C_NUMZERO];
    report->lastzero = (int64_t) h[C_LASTZERO] - 1;
    report->numprob = (int64_t) h[C_NUMPROB];
    report->lastprob = (int64_t) h[C_LASTPROB] - 1;
    report->nbad_delaytime = (int64_t) h[C_NBADDELAY];
    report->first_bad_delaytime = h[C_FIRST_BADDELAY] == ST_NONE ? -1 : (int64_t) h[C_FIRST_BADDELAY];
    return SHQ_OK;
}

extern "C" int shq_startup_check_density_entropy(shq_context *ctx, const shq_startup_layout *layout, void *d_sph, int64_t nsph, double meanbar, double MinEgySpec,
                                                 double atime, int64_t *bad)
{
    SHQ_CHECK(ctx && layout && bad, SHQ_ERR_INVALID, "null argument");
    SHQ_TRY(check_sph_layout(layout, d_sph, nsph, false));
    *bad = 0;
    if(nsph == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(st_reset(ctx));
    const double a3 = pow(atime, 3);
    st_density_entropy_kernel<<<dim3(nblk(nsph)), dim3(256), 0, ctx->stream>>>(*layout, (char *) d_sph, (long long) nsph, meanbar, MinEgySpec, a3,
                                                                              reinterpret_cast<unsigned long long *>(ctx->st_cnt.ptr));
    SHQ_HIP(hipGetLastError());
    unsigned long long h[C_N];
    SHQ_TRY(st_counters(ctx, h));
    *bad = (int64_t) h[C_BADDENS];
    return SHQ_OK;
}

/* the loop; bad[] = particles that met "Bad tree moments", "Bad hsml guess", "Bad init father" */
static int set_init_hsml_counted(shq_context *ctx, double MeanGasSeparation, double DesNumNgb, int32_t *d_node_out, unsigned long long bad[3])
{
    bad[0] = bad[1] = bad[2] = 0;
    SHQ_CHECK(ctx->have_parts && ctx->have_types && (ctx->have_dyn || ctx->have_sph), SHQ_ERR_STATE,
              "set_init_hsml: upload the particles with their Type, and Hsml (shq_dynamics_upload or an SPH state), first");
    SHQ_CHECK(ctx->have_tree && ctx->have_father, SHQ_ERR_STATE, "tree Father array not allocated at initial hsml!");
    const long long n = ctx->numpart;
    SHQ_CHECK(n == 0 || (ctx->hsml.cap >= (size_t) n && ctx->pfather.cap >= (size_t) n && ctx->node_father.cap > (size_t) ctx->numnodes), SHQ_ERR_STATE,
              "set_init_hsml: the resident arrays do not cover the particles");
    if(n == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SHQ_TRY(st_reset(ctx));
    const int32_t *order = nullptr;
    if(d_node_out && !ctx->node_order.empty()) { /* an uploaded tree: the pool is in walk order, the caller's numbers are not */
        SHQ_TRY(ctx->st_i32.reserve(ctx->node_order.size()));
        SHQ_HIP(hipMemcpyAsync(ctx->st_i32.ptr, ctx->node_order.data(), sizeof(int32_t) * ctx->node_order.size(), hipMemcpyHostToDevice, st));
        order = ctx->st_i32.ptr;
    }
    st_init_hsml_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, ctx->posm.ptr, ctx->pflags.ptr, ctx->pfather.ptr, ctx->node_father.ptr, ctx->nodeA.ptr, ctx->nodeB.ptr,
                                                             (long long) ctx->numnodes, MeanGasSeparation, DesNumNgb, ctx->treeBox, ctx->hsml.ptr, d_node_out, order,
                                                             (long long) ctx->firstnode, reinterpret_cast<unsigned long long *>(ctx->st_cnt.ptr));
    SHQ_HIP(hipGetLastError());
    unsigned long long h[C_N];
    SHQ_TRY(st_counters(ctx, h));
    ctx->inputs_current &= ~SHQ_CURRENT_SPH; /* the resident Hsml is no longer the caller's */
    bad[0] = h[C_BADMOM];
    bad[1] = h[C_BADHSML];
    bad[2] = h[C_BADCHAIN];
    return SHQ_OK;
}

extern "C" int shq_set_init_hsml(shq_context *ctx, double MeanGasSeparation, double DesNumNgb, int32_t *d_node_out)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    unsigned long long bad[3];
    SHQ_TRY(set_init_hsml_counted(ctx, MeanGasSeparation, DesNumNgb, d_node_out, bad));
    SHQ_CHECK(bad[2] == 0, SHQ_ERR_INVALID, "Bad init father: %llu particles with a father outside the tree or a chain longer than %d", bad[2], ST_MAXCLIMB);
    SHQ_CHECK(bad[0] == 0, SHQ_ERR_INVALID, "Bad tree moments: %llu particles ended on a node longer than the box or lighter than themselves", bad[0]);
    SHQ_CHECK(bad[1] == 0, SHQ_ERR_INVALID, "Bad hsml guess: %llu particles with Hsml <= 0", bad[1]);
    return SHQ_OK;
}

extern "C" int shq_init_entropy(shq_context *ctx, double u_init, double a3, int from_egywt)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    SHQ_CHECK(ctx->have_parts && ctx->have_types && ctx->have_sph, SHQ_ERR_STATE, "init_entropy: no SPH state on the device");
    const long long n = ctx->numpart;
    if(n == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    if(from_egywt)
        SHQ_TRY(ctx->st_old.reserve((size_t) n));
    st_entropy_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(n, ctx->pflags.ptr, from_egywt ? ctx->g_egywt.ptr : ctx->g_density.ptr, ctx->g_entropy.ptr,
                                                                   from_egywt ? ctx->st_old.ptr : nullptr, u_init, a3);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* shq_entropy_download copies outside the stream */
    ctx->inputs_current &= ~SHQ_CURRENT_SPH;
    return SHQ_OK;
}

extern "C" int shq_setup_smoothinglengths(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const shq_bh_view *bh, const shq_startup_sml_params *params,
                                          shq_startup_sml_stats *stats)
{
    SHQ_CHECK(ctx && parts && sph && params, SHQ_ERR_INVALID, "null argument");
    if(stats)
        memset(stats, 0, sizeof(*stats));
    if(sph->numslots + (bh ? bh->numslots : 0) == 0) /* a pure dark-matter run */
        return SHQ_OK;
    SHQ_CHECK(parts->off_type != SHQ_NOFIELD && parts->off_pi != SHQ_NOFIELD && parts->off_hsml != SHQ_NOFIELD, SHQ_ERR_INVALID,
              "setup_smoothinglengths needs Type, PI and Hsml in the particle view");
    SHQ_CHECK(params->atime > 0 && std::isfinite(params->atime), SHQ_ERR_INVALID, "setup_smoothinglengths: atime = %g", params->atime);
    SHQ_CHECK(ctx->sphrun.phase == 0, SHQ_ERR_STATE, "setup_smoothinglengths: another SPH walk is open");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int64_t n = parts->numpart;
    /* the work queue: DensityQuery::haswork for every particle, as at the first step all are active */
    std::vector<int32_t> &queue = ctx->sph_queue_host;
    queue.clear();
    for(int64_t i = 0; i < n; i++) {
        if(parts->off_flags != SHQ_NOFIELD && (*hfield<uint32_t>(parts, i, parts->off_flags) & 3u))
            continue;
        const uint8_t t = *hfield<uint8_t>(parts, i, parts->off_type);
        if(t != 0 && t != 5)
            continue;
        const int32_t pi = *hfield<int32_t>(parts, i, parts->off_pi);
        if(t == 5)
            SHQ_CHECK(bh && bh->base && pi >= 0 && pi < bh->numslots, SHQ_ERR_INVALID, "BH particle with PI outside the BH slot array");
        queue.push_back((int32_t) i);
    }
    const int64_t nq = (int64_t) queue.size();
    /* the one upload */
    SHQ_TRY(shq_particles_upload(ctx, parts));
    SHQ_TRY(shq_sph_state_upload(ctx, parts, sph));
    SHQ_TRY(ctx->s_queue0.reserve((size_t) std::max<int64_t>(nq, 1)));
    if(nq > 0)
        SHQ_HIP(hipMemcpyAsync(ctx->s_queue0.ptr, queue.data(), sizeof(int32_t) * nq, hipMemcpyHostToDevice, st));
    /* finds fathers for each gas and BH particle, so the tree needs the BHs */
    const double Box = params->density.BoxSize;
    int rc = shq_tree_build(ctx, Box, (1 << 0) + (1 << 5), nullptr, 0, nullptr);
    unsigned long long bad[3] = {0, 0, 0};
    if(rc == SHQ_OK)
        rc = set_init_hsml_counted(ctx, params->MeanGasSeparation, params->density.DesNumNgb, nullptr, bad);
    if(rc == SHQ_OK && bad[2]) {
        shq_set_error("Bad init father: %llu particles with a father outside the tree or a chain longer than %d", bad[2], ST_MAXCLIMB);
        rc = SHQ_ERR_INVALID;
    }
    if(stats) { /* reported, not enforced: the caller decides (the reference ends the run) */
        stats->nbad_moments = (int64_t) bad[0];
        stats->nbad_hsml = (int64_t) bad[1];
    }
    shq_density_params dp = params->density;
    const double a3 = pow(params->atime, 3);
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(ctx->st_cnt.ptr);
    int nrounds = 0, nmaxdiff = 0;
    if(rc == SHQ_OK) {
        dp.update_hsml = 1;
        dp.DoEgyDensity = 0;
        rc = shq_sph_prepare(ctx, &dp.kf, nullptr, nullptr);
        if(rc == SHQ_OK)
            rc = shq_sph_density_device(ctx, &dp, ctx->s_queue0.ptr, nq, 0, stats ? &stats->first : nullptr);
    }
    if(rc == SHQ_OK && !params->DensityIndependentSphOn)
        rc = shq_init_entropy(ctx, params->u_init, a3, 0); /* initialise to the initial energy */
    if(rc == SHQ_OK && params->DensityIndependentSphOn && n > 0) {
        /* better convergence than initialising EgyWtDensity before Density is known */
        SHQ_HIP(hipMemcpyAsync(ctx->g_egywt.ptr, ctx->g_density.ptr, sizeof(double) * (size_t) n, hipMemcpyDeviceToDevice, st));
        dp.update_hsml = 0;
        dp.DoEgyDensity = 1;
        int stop = 0;
        for(int j = 0; j < 100 && rc == SHQ_OK; j++) {
            /* the initial conditions give energies, not entropies: iterate */
            rc = shq_init_entropy(ctx, params->u_init, a3, 1);
            if(rc == SHQ_OK)
                rc = shq_sph_prepare(ctx, &dp.kf, nullptr, nullptr);
            if(rc == SHQ_OK)
                rc = shq_sph_density_device(ctx, &dp, ctx->s_queue0.ptr, nq, 0, nullptr);
            if(rc != SHQ_OK)
                break;
            nrounds++;
            if(stop)
                break;
            SHQ_TRY(st_reset(ctx));
            st_maxdiff_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, ctx->pflags.ptr, ctx->g_egywt.ptr, ctx->st_old.ptr, cnt);
            SHQ_HIP(hipGetLastError());
            unsigned long long h[C_N];
            SHQ_TRY(st_counters(ctx, h));
            double maxdiff;
            memcpy(&maxdiff, &h[C_MAXDIFF], sizeof(double));
            if(stats)
                stats->maxdiff[nmaxdiff] = maxdiff;
            nmaxdiff++;
            if(maxdiff < 1e-3) /* one more iteration, then stop */
                stop = 1;
        }
    }
    /* no tree stays installed: the reference frees it */
    ctx->have_tree = false;
    ctx->tb_built = false;
    ctx->have_tree_targets = false;
    ctx->sphrun.phase = 0;
    ctx->inputs_current = 0;
    if(rc != SHQ_OK)
        return rc;
    if(stats) {
        stats->nrounds = nrounds;
        stats->nmaxdiff = nmaxdiff;
    }
    /* one write-back, for the walked targets only (reduce<PRIMARY>, localtreewalk2.h:39) */
    const size_t cap = (size_t) std::max<int64_t>(n, 1);
    SHQ_TRY(ctx->stage.reserve(cap * 8 * sizeof(double) + 256));
    double *col[8];
    const double *src[8] = {ctx->hsml.ptr, ctx->dthsml.ptr, ctx->g_density.ptr, ctx->g_egywt.ptr, ctx->g_dhsmlegy.ptr, ctx->g_divvel.ptr, ctx->g_curlvel.ptr,
                            ctx->g_entropy.ptr};
    for(int c = 0; c < 8; c++) {
        col[c] = reinterpret_cast<double *>(ctx->stage.ptr) + (size_t) c * cap;
        if(n > 0)
            SHQ_HIP(hipMemcpyAsync(col[c], src[c], sizeof(double) * (size_t) n, hipMemcpyDeviceToHost, st));
    }
    SHQ_HIP(hipStreamSynchronize(st));
    /* set_init_hsml wrote every gas and black-hole particle that is not garbage, a swallowed black hole included */
    for(int64_t i = 0; i < n; i++) {
        const uint8_t t = *hfield<uint8_t>(parts, i, parts->off_type);
        if((t == 0 || t == 5) && !(parts->off_flags != SHQ_NOFIELD && (*hfield<uint32_t>(parts, i, parts->off_flags) & 1u)))
            *hfield<double>(parts, i, parts->off_hsml) = col[0][i];
    }
    auto slot = [&](int32_t pi, size_t off) { return reinterpret_cast<double *>(static_cast<char *>(sph->base) + (size_t) pi * sph->elsize + off); };
    for(int32_t i : queue) {
        *hfield<double>(parts, i, parts->off_hsml) = col[0][i];
        if(parts->off_dthsml != SHQ_NOFIELD)
            *hfield<double>(parts, i, parts->off_dthsml) = col[1][i];
        const uint8_t t = *hfield<uint8_t>(parts, i, parts->off_type);
        const int32_t pi = *hfield<int32_t>(parts, i, parts->off_pi);
        if(t == 0) {
            *slot(pi, sph->off_density) = col[2][i];
            *slot(pi, sph->off_egywtdensity) = col[3][i];
            *slot(pi, sph->off_dhsmlegydensityfactor) = col[4][i];
            *slot(pi, sph->off_divvel) = col[5][i];
            *slot(pi, sph->off_curlvel) = col[6][i];
            *slot(pi, sph->off_entropy) = col[7][i];
        } else {
            char *b = static_cast<char *>(bh->base) + (size_t) pi * bh->elsize;
            *reinterpret_cast<double *>(b + bh->off_density) = col[2][i];
            *reinterpret_cast<double *>(b + bh->off_divvel) = col[5][i];
        }
    }
    return SHQ_OK;
}
