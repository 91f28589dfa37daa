/* heiii.hip — helium reionisation by quasar bubbles on the device for one rank: turn_on_quasars (libgadget/cooling_qso_lightup.cpp:489-596)
 * with the legacy neighbour walk it runs per quasar (ionize_all_part, :442-483; treewalk.c:905-1122).
 *
 * The reference lights one quasar at a time: draw a candidate, walk the gas tree for the particles inside its bubble, flag and heat them,
 * update the HeIII fraction, stop when it reaches the target.  Which quasars are drawn does not depend on what they ionise (only on the
 * random table and the candidate count), so the draws are made up front on the host, and the loop becomes:
 *  - the candidate groups are compacted from the resident FOF catalogue on the device; only (index, MinID, CM) comes down;
 *  - the host draws a batch of quasars (positions, radii with glibc's log / cos / sqrt, the end of the candidate list) and uploads the
 *    lit bubbles in sequence order;
 *  - one lane per still-eligible gas particle records the FIRST bubble of the batch that holds it (a particle ionised by bubble j is no
 *    longer eligible for any later one, so that is the bubble that ionises it in the serial loop); per-bubble counts go through an LDS
 *    histogram per workgroup and one global integer add per (workgroup, bubble);
 *  - the host replays the loop's control over the batch's counts and finds the last iteration that runs; the particles whose first hit is
 *    at or before it are flagged and heated and leave the eligible list; if the loop has not stopped, the next batch (twice as many draws,
 *    up to HEIII_MAX_BATCH) sweeps the rest.
 *
 * Membership of a gas particle in bubble (CM, R) is the walk's particle test, !(r2 > R*R) with r2 summed in x, y, z order of
 * NEAREST(CM - Pos) (the walk's early exit once r2 > R*R cannot change the outcome: the partial sums only grow).  For R >= 0 or NaN the
 * walk's node test (cull_node, treewalk.c:990-1019) never rejects the node of a particle that passes, so the particle test decides.  For
 * R < 0 it does not; then the leaf of the particle (Father) and every node above it must pass cull_node as well, with its arithmetic.
 *
 * Quirks of the reference that are kept (one task):
 *  - the candidate at remaining-list position 0 is drawn and erased but never walked (ionize_all_part walks only for qso_ind > 0): it
 *    counts as an iteration and logs position (0, 0, 0);
 *  - the draw that leaves no candidate (ncand_tot <= 0 after the decrement) ends the loop before it ionises: the last candidate is never lit;
 *  - choose_QSO_halo's bookkeeping is replayed as written (ncand_before starts at 0; a draw off the list is -1: no walk, no erase);
 *  - u1 = 0 in gaussian_rng gives an infinite or NaN radius, which takes every eligible gas particle (or, at -inf, none);
 *  - the flash-ionisation loop takes every Type-0 particle below NumPart, garbage included, and the initial fraction counts them too;
 *  - the "insufficient ionisation" stop compares with 0.01 * non_overlapping_bubble_number as the reference forms it (cgs constants with
 *    internal lengths): it is 0 for physical inputs and never fires.
 * What differs: the ionised particles are flagged in one pass per batch instead of one walk per quasar (same particles, same entropies:
 * every particle is heated once, from its own slot's Density); the gas tree is assumed to hold every live gas particle, as the tree of
 * run.cpp:482 / 624 does (the walk would miss one that is not in it).
 */
#include "call_scope.hpp"
#include "device_prims.hpp"
#include <rocprim/iterator/transform_iterator.hpp>
#include <math.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>

/* physconst.h, cooling_qso_lightup.cpp:48, treewalk.c:19 */
#define HEIII_HYDROGEN_MASSFRAC 0.76
#define HEIII_PROTONMASS 1.6726e-24
#define HEIII_HEMASS 4.002602
#define HEIII_GAMMA_MINUS1 ((5.0 / 3.0) - 1)
#define HEIII_HUBBLE 3.2407789e-18
#define HEIII_GRAVITY 6.672e-8
#define HEIII_FACT1 0.366025403785

namespace {

/* libm through pointers the compiler cannot see through: the radii and the bubble-count threshold must be what glibc returns */
double (*volatile libm_log)(double) = log;
double (*volatile libm_cos)(double) = cos;
double (*volatile libm_sqrt)(double) = sqrt;
double (*volatile libm_pow)(double, double) = pow;

constexpr int HT = 256;
constexpr int HEIII_FIRST_BATCH = 32;
constexpr int HEIII_MAX_BATCH = 1024;   /* draws per sweep; the LDS histogram holds one counter per lit bubble */
constexpr int HEIII_SWEEP_BLOCKS = 4096; /* grid-stride cap of the sweep: the histogram is flushed once per workgroup */
constexpr int HEIII_MAX_DEPTH = 4096;   /* guard of the ancestor chain (a tree is far shallower) */

struct Bubble {      /* one lit quasar, 48 bytes, read by wave-uniform loads */
    double c[3];
    double R, R2;    /* radius and R * R (the walk's h2) */
    int32_t neg;     /* R < 0: the ancestors' cull_node decides as well */
    int32_t pad_;
};
struct CandRow {     /* a candidate group */
    int64_t group;
    uint64_t minid;
    double cm[3];
};

__device__ __forceinline__ double nearest(double x, double box)
{
    return x > 0.5 * box ? x - box : (x < -0.5 * box ? x + box : x); /* NEAREST, partmanager.h:99 */
}

/* the nodes a walk for a bubble of radius R < 0 passes through on its way to the leaf of the particle: all must pass cull_node */
__device__ bool chain_passes(int node, const Bubble &b, double box, const NodeB *__restrict__ nodeB, const int32_t *__restrict__ nfather)
{
#pragma clang fp contract(off)
    if(node < 0)
        return false; /* not in the tree: no walk finds it */
    for(int depth = 0; node >= 0 && depth < HEIII_MAX_DEPTH; depth++) {
        const NodeB nb = nodeB[node];
        double dist = b.R + 0.5 * nb.len;
        double r2 = 0;
        for(int d = 0; d < 3; d++) {
            const double dx = nearest(nb.center[d] - b.c[d], box);
            if(dx > dist)
                return false;
            if(dx < -dist)
                return false;
            r2 += dx * dx;
        }
        dist += HEIII_FACT1 * nb.len;
        if(r2 > dist * dist)
            return false;
        node = nfather[node];
    }
    return node < 0;
}

/* one lane per eligible particle: the first lit bubble of the batch that holds it (-1: none); per-bubble counts */
__global__ __launch_bounds__(HT) void heiii_sweep_kernel(long long m, const double4 *__restrict__ elig, const Bubble *__restrict__ bub, int nb,
                                                         double box, const NodeB *__restrict__ nodeB, const int32_t *__restrict__ nfather,
                                                         const int32_t *__restrict__ pfather, int32_t *__restrict__ hit,
                                                         unsigned long long *__restrict__ counts)
{
#pragma clang fp contract(off)
    extern __shared__ unsigned hist[];
    for(int k = threadIdx.x; k < nb; k += HT)
        hist[k] = 0;
    __syncthreads();
    for(long long i0 = (long long) blockIdx.x * HT; i0 < m; i0 += (long long) gridDim.x * HT) {
        const long long i = i0 + threadIdx.x;
        int h = -1;
        if(i < m) {
            const double4 e = elig[i];
            for(int k = 0; k < nb; k++) {
                const Bubble b = bub[k];
                const double dx = nearest(b.c[0] - e.x, box);
                const double dy = nearest(b.c[1] - e.y, box);
                const double dz = nearest(b.c[2] - e.z, box);
                double r2 = dx * dx;
                r2 += dy * dy;
                r2 += dz * dz;
                if(!(r2 > b.R2) && (!b.neg || chain_passes(pfather[(int) e.w], b, box, nodeB, nfather))) {
                    h = k;
                    break;
                }
            }
            hit[i] = h;
        }
        if(h >= 0)
            atomicAdd(&hist[h], 1u);
    }
    __syncthreads();
    for(int k = threadIdx.x; k < nb; k += HT)
        if(hist[k])
            atomicAdd(&counts[k], (unsigned long long) hist[k]);
}

/* ionize_single_particle (:354-373) for a list of particles that are not ionised yet: flag, heat, and one row (index, new Entropy) each
 * for the caller's records */
__device__ __forceinline__ void heat_one(int p, uint8_t *pflags, double *entropy, const double *__restrict__ density, double a3inv, double du,
                                         double2 *row)
{
#pragma clang fp contract(off)
    pflags[p] = (uint8_t) (pflags[p] | SHQ_FLAG_HEIII);
    const double entropytou = pow(density[p] * a3inv, HEIII_GAMMA_MINUS1) / HEIII_GAMMA_MINUS1;
    const double e = entropy[p] + du / entropytou;
    entropy[p] = e;
    *row = make_double2((double) p, e);
}
__global__ void heiii_apply_rec_kernel(long long m, const double4 *__restrict__ rec, uint8_t *pflags, double *entropy, const double *__restrict__ density,
                                       double a3inv, double du, double2 *rows)
{
    const long long i = (long long) blockIdx.x * HT + threadIdx.x;
    if(i < m)
        heat_one((int) rec[i].w, pflags, entropy, density, a3inv, du, rows + i);
}
__global__ void heiii_apply_idx_kernel(long long m, const int32_t *__restrict__ idx, uint8_t *pflags, double *entropy, const double *__restrict__ density,
                                       double a3inv, double du, double2 *rows)
{
    const long long i = (long long) blockIdx.x * HT + threadIdx.x;
    if(i < m)
        heat_one(idx[i], pflags, entropy, density, a3inv, du, rows + i);
}

/* gas_ionization_fraction's count (:334-341): Type 0 with the flag, garbage included */
__global__ __launch_bounds__(HT) void heiii_count_kernel(long long n, const uint8_t *__restrict__ pflags, unsigned long long *count)
{
    const long long i = (long long) blockIdx.x * HT + threadIdx.x;
    const unsigned f = i < n ? pflags[i] : 0x10u;
    const int c = __syncthreads_count((f >> 4) == 0 && (f & SHQ_FLAG_HEIII));
    if(threadIdx.x == 0 && c)
        atomicAdd(count, (unsigned long long) c);
}

__global__ void heiii_gather_kernel(long long m, const int32_t *__restrict__ idx, const double4 *__restrict__ posm, double4 *out)
{
    const long long i = (long long) blockIdx.x * HT + threadIdx.x;
    if(i < m) {
        const int p = idx[i];
        const double4 x = posm[p];
        out[i] = make_double4(x.x, x.y, x.z, (double) p);
    }
}

__global__ void heiii_cand_kernel(long long m, const int32_t *__restrict__ idx, const shq_fof_group *__restrict__ groups, CandRow *out)
{
    const long long i = (long long) blockIdx.x * HT + threadIdx.x;
    if(i < m) {
        const int g = idx[i];
        CandRow r;
        r.group = g;
        r.minid = groups[g].MinID;
        for(int d = 0; d < 3; d++)
            r.cm[d] = groups[g].CM[d];
        out[i] = r;
    }
}

/* father of every node of the packed tree (pre-order): the children of an internal node are its first child and that child's siblings up
 * to the node's own sibling (the threaded layout, forcetree.cpp:1016-1103) */
__global__ void heiii_node_father_kernel(long long nn, const NodeC *__restrict__ nodeC, int32_t *nfather)
{
    const long long i = (long long) blockIdx.x * HT + threadIdx.x;
    if(i >= nn)
        return;
    const NodeC c = nodeC[i];
    if(c.type != SHQ_NODE_NODE_TYPE)
        return;
    int ch = c.child;
    for(int k = 0; k < SHQ_NMAXCHILD && ch >= 0 && ch < nn && ch != c.sibling; k++) {
        nfather[ch] = (int32_t) i;
        ch = nodeC[ch].sibling;
    }
}

struct InWindow {     /* build_qso_candidate_list (:260-276) */
    const shq_fof_group *groups;
    double lo, hi;
    __device__ bool operator()(const int32_t &g) const { return !(groups[g].Mass < lo) && !(groups[g].Mass > hi); }
};
struct Eligible {     /* what the walk can ionise: gas, not garbage, not yet ionised */
    const uint8_t *pflags;
    __device__ bool operator()(const int32_t &i) const { const unsigned f = pflags[i]; return (f >> 4) == 0 && !(f & (1u | SHQ_FLAG_HEIII)); }
};
struct Flashable {    /* the flash loop (:506-510): every Type-0 particle not ionised yet */
    const uint8_t *pflags;
    __device__ bool operator()(const int32_t &i) const { const unsigned f = pflags[i]; return (f >> 4) == 0 && !(f & SHQ_FLAG_HEIII); }
};
struct HitBefore {    /* first hit among the bubbles the loop ran */
    int kstop;
    __device__ bool operator()(const int32_t &h) const { return h >= 0 && h < kstop; }
};

} // namespace

extern "C" int shq_heiii_last_stats(shq_context *ctx, shq_heiii_stats *stats)
{
    SHQ_CHECK(ctx && stats, SHQ_ERR_INVALID, "null argument");
    *stats = ctx->heiii_stats;
    return SHQ_OK;
}

extern "C" int shq_heiii_reionization(shq_context *ctx, const shq_heiii_params *p, const shq_part_view *parts, const shq_sph_view *sph,
                                      const shq_tree_view *gas_tree, const double *rnd_table, int64_t rnd_size, shq_heiii_quasar *log,
                                      int64_t log_capacity, int64_t *nlog, shq_heiii_result *result)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx && p && parts && sph && rnd_table && result, SHQ_ERR_INVALID, "heiii: null argument");
    SHQ_CHECK(rnd_size > 0, SHQ_ERR_INVALID, "heiii: empty random table");
    SHQ_CHECK(log_capacity >= 0 && (log || log_capacity == 0), SHQ_ERR_INVALID, "heiii: bad log buffer");
    SHQ_CHECK(p->BoxSize > 0 && p->atime > 0 && p->n_gas_tot > 0, SHQ_ERR_INVALID, "heiii: BoxSize, atime and n_gas_tot must be > 0");
    SHQ_CHECK(parts->off_pos != SHQ_NOFIELD && parts->off_type != SHQ_NOFIELD && parts->off_flags != SHQ_NOFIELD && parts->off_pi != SHQ_NOFIELD,
              SHQ_ERR_INVALID, "heiii: the particle view needs Pos, Type, PI and the flag byte");
    SHQ_CHECK(sph->off_density != SHQ_NOFIELD && sph->off_entropy != SHQ_NOFIELD, SHQ_ERR_INVALID, "heiii: the gas view needs Density and Entropy");
    /* a negative radius makes membership depend on the tree (cull_node): a positive variance, or a negative mean, needs it */
    const bool need_tree = !(p->var_bubble <= 0) || p->mean_bubble < 0;
    SHQ_CHECK(!need_tree || (gas_tree && gas_tree->father), SHQ_ERR_INVALID, "heiii: var_bubble > 0 needs the gas tree with its father array");
    SHQ_CHECK(ctx->fof_ngroups >= 0, SHQ_ERR_STATE, "heiii: no FOF catalogue (run shq_fof first)");
    SHQ_CHECK(ctx->sphrun.phase == 0, SHQ_ERR_STATE, "heiii: an SPH walk is open");
    SHQ_HIP(hipSetDevice(ctx->device));
    memset(result, 0, sizeof(*result));
    if(nlog)
        *nlog = 0;
    shq_heiii_stats st;
    memset(&st, 0, sizeof(st));
    hipStream_t s = ctx->stream;
    CallScope sc(ctx, "heiii");
    SHQ_TRY(sc.mark(s));
    unsigned long long *d_cnt;
    SHQ_TRY(sc.alloc(&d_cnt, 2));

    /* ---- candidates, from the catalogue as it is now: a particle upload below drops it */
    const int64_t TotNgroups = ctx->fof_ngroups;
    std::vector<CandRow> cand;
    {
        int32_t *gidx;
        CandRow *rows;
        SHQ_TRY(sc.alloc(&gidx, (size_t) TotNgroups));
        int64_t K = 0;
        SHQ_TRY(prim_select_if(ctx, rocprim::counting_iterator<int32_t>(0), gidx, (size_t) TotNgroups,
                               InWindow{ctx->fof_groups.ptr, p->qso_candidate_min_mass, p->qso_candidate_max_mass}, d_cnt, &K));
        SHQ_TRY(sc.alloc(&rows, (size_t) K));
        if(K > 0) {
            heiii_cand_kernel<<<dim3(nblk(K, HT)), dim3(HT), 0, s>>>(K, gidx, ctx->fof_groups.ptr, rows);
            SHQ_HIP(hipGetLastError());
            cand.resize((size_t) K);
            SHQ_HIP(hipMemcpyAsync(cand.data(), rows, sizeof(CandRow) * (size_t) K, hipMemcpyDeviceToHost, s));
            SHQ_HIP(hipStreamSynchronize(s));
        }
    }

    /* ---- particles and their gas state: uploaded, or the context's copies when the caller vouches for them */
    SHQ_TRY(shq_particles_upload(ctx, parts));
    SHQ_TRY(shq_sph_state_upload(ctx, parts, sph));
    const long long n = parts->numpart;
    uint8_t *d_flags = ctx->pflags.ptr;
    double *d_entropy = ctx->g_entropy.ptr;
    const double *d_density = ctx->g_density.ptr;

    const double a3inv = 1 / libm_pow(p->atime, 3);
    const double nheperg = (1 - HEIII_HYDROGEN_MASSFRAC) / (HEIII_PROTONMASS * HEIII_HEMASS);
    const double deltau = p->qso_inst_heating * nheperg;
    const double du = deltau / p->uu_in_cgs;
    const double ngas = (double) p->n_gas_tot;

    double2 *d_rows; /* (index, new Entropy) of every particle ionised by this call */
    SHQ_TRY(sc.alloc(&d_rows, (size_t) n));
    int64_t nrows = 0;

    /* ---- flash ionisation (:501-512) */
    if(p->desired_ion_frac > p->heIIIreion_finish_frac) {
        int32_t *fidx;
        SHQ_TRY(sc.alloc(&fidx, (size_t) n));
        int64_t nf = 0;
        SHQ_TRY(prim_select_if(ctx, rocprim::counting_iterator<int32_t>(0), fidx, (size_t) n, Flashable{d_flags}, d_cnt, &nf));
        if(nf > 0) {
            heiii_apply_idx_kernel<<<dim3(nblk(nf, HT)), dim3(HT), 0, s>>>(nf, fidx, d_flags, d_entropy, d_density, a3inv, du, d_rows);
            SHQ_HIP(hipGetLastError());
        }
        nrows = nf;
        result->n_flash = nf;
    }

    /* ---- gas_ionization_fraction (:330-346) and the bubble-count threshold (:514-518) */
    SHQ_HIP(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), s));
    if(n > 0) {
        heiii_count_kernel<<<dim3(nblk(n, HT)), dim3(HT), 0, s>>>(n, d_flags, d_cnt);
        SHQ_HIP(hipGetLastError());
    }
    unsigned long long nion0 = 0;
    SHQ_HIP(hipMemcpyAsync(&nion0, d_cnt, sizeof(nion0), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    const double initionfrac = (double) nion0 / ngas;
    double curionfrac = initionfrac;
    const double rhobar = p->OmegaBaryon * (3 * HEIII_HUBBLE * p->HubbleParam * HEIII_HUBBLE * p->HubbleParam) / (8 * M_PI * HEIII_GRAVITY) * a3inv;
    const double totbubblegasmass = 4 * M_PI / 3. * libm_pow(p->mean_bubble, 3) * rhobar;
    const int64_t non_overlapping_bubble_number = (int64_t) (p->n_gas_tot * totbubblegasmass / p->OmegaBaryon);
    result->init_ionfrac = initionfrac;
    if(!(curionfrac < p->desired_ion_frac))
        cand.clear(); /* the candidate list is built only below the target */
    const int64_t K = (int64_t) cand.size();
    result->n_candidates = K;

    int64_t iteration = 0, tot_n_ionized = 0;
    if(K > 0) {
        /* ---- the eligible gas, as records (x, y, z, index) the sweeps stream */
        int32_t *eidx, *d_hit, *d_nfather = nullptr;
        double4 *E[2], *S;
        Bubble *d_bub;
        unsigned long long *d_counts;
        SHQ_TRY(sc.alloc(&eidx, (size_t) n));
        int64_t m = 0;
        SHQ_TRY(prim_select_if(ctx, rocprim::counting_iterator<int32_t>(0), eidx, (size_t) n, Eligible{d_flags}, d_cnt, &m));
        SHQ_TRY(sc.alloc(&E[0], (size_t) m));
        SHQ_TRY(sc.alloc(&E[1], (size_t) m));
        SHQ_TRY(sc.alloc(&S, (size_t) m));
        SHQ_TRY(sc.alloc(&d_hit, (size_t) m));
        SHQ_TRY(sc.alloc(&d_bub, HEIII_MAX_BATCH));
        SHQ_TRY(sc.alloc(&d_counts, HEIII_MAX_BATCH));
        if(m > 0) {
            heiii_gather_kernel<<<dim3(nblk(m, HT)), dim3(HT), 0, s>>>(m, eidx, ctx->posm.ptr, E[0]);
            SHQ_HIP(hipGetLastError());
        }
        st.neligible = m;
        SHQ_TRY(sc.mark(s));
        SHQ_HIP(hipEventSynchronize(sc.ev.back()));
        st.ms[0] = sc.last_ms();
        int cur = 0;
        bool tree_ready = false;

        /* the reference's candidate list and choose_QSO_halo's counters (:314-328, one task: ncand_before starts at 0) */
        std::vector<int32_t> qso_cand((size_t) K);
        std::iota(qso_cand.begin(), qso_cand.end(), 0);
        int64_t ncand_tot = K, ncand_before = 0;
        const double sigma = libm_sqrt(p->var_bubble);
        bool seq_end = false, stopped = false;
        int batch = HEIII_FIRST_BATCH;
        struct Draw {
            int32_t cand; /* index into cand[], -1: nothing walked */
        };
        std::vector<Draw> draws;
        std::vector<Bubble> hb;
        std::vector<unsigned long long> counts(HEIII_MAX_BATCH);
        while(!stopped && !seq_end) {
            /* ---- draw the next batch: positions, radii, the end of the list */
            draws.clear();
            hb.clear();
            bool any_neg = false;
            for(int d = 0; d < batch; d++) {
                const double drand = rnd_table[(uint64_t) (TotNgroups + iteration + d) % (uint64_t) rnd_size];
                const int64_t qso = drand * ncand_tot;
                ncand_tot--;
                if(qso < ncand_before)
                    ncand_before--;
                const int64_t new_qso = (qso < ncand_before || qso >= ncand_before + (int64_t) qso_cand.size()) ? -1 : qso - ncand_before;
                if(ncand_tot <= 0) { /* "not enough quasars": the loop ends before this one */
                    seq_end = true;
                    break;
                }
                Draw dr{-1};
                if(new_qso > 0) {
                    dr.cand = qso_cand[(size_t) new_qso];
                    const CandRow &c = cand[(size_t) dr.cand];
                    /* gaussian_rng(mean, sqrt(var), MinID) (:249-255) */
                    const double u1 = rnd_table[c.minid % (uint64_t) rnd_size];
                    const double u2 = rnd_table[(c.minid + 1) % (uint64_t) rnd_size];
                    const double z1 = libm_sqrt(-2 * libm_log(u1)) * libm_cos(2 * M_PI * u2);
                    Bubble b;
                    memset(&b, 0, sizeof(b));
                    for(int k = 0; k < 3; k++)
                        b.c[k] = c.cm[k];
                    b.R = p->mean_bubble + sigma * z1;
                    b.R2 = b.R * b.R;
                    b.neg = b.R < 0;
                    any_neg |= b.neg != 0;
                    hb.push_back(b);
                }
                draws.push_back(dr);
                if(new_qso >= 0) /* erased whatever happens, unless the loop stops at it (then it no longer matters) */
                    qso_cand.erase(qso_cand.begin() + new_qso);
            }
            const int L = (int) hb.size();
            std::fill(counts.begin(), counts.end(), 0ull);
            /* ---- sweep the eligible gas against the batch's lit bubbles */
            if(L > 0 && m > 0) {
                if(any_neg && !tree_ready) {
                    SHQ_TRY(shq_tree_upload(ctx, gas_tree));
                    SHQ_CHECK(ctx->have_father, SHQ_ERR_INVALID, "heiii: the gas tree has no father array");
                    const long long nn = ctx->numnodes;
                    SHQ_TRY(sc.alloc(&d_nfather, (size_t) nn));
                    SHQ_HIP(hipMemsetAsync(d_nfather, 0xff, sizeof(int32_t) * (size_t) nn, s));
                    heiii_node_father_kernel<<<dim3(nblk(nn, HT)), dim3(HT), 0, s>>>(nn, ctx->nodeC.ptr, d_nfather);
                    SHQ_HIP(hipGetLastError());
                    tree_ready = true;
                }
                SHQ_HIP(hipMemcpyAsync(d_bub, hb.data(), sizeof(Bubble) * (size_t) L, hipMemcpyHostToDevice, s));
                SHQ_HIP(hipMemsetAsync(d_counts, 0, sizeof(unsigned long long) * (size_t) L, s));
                SHQ_TRY(sc.mark(s));
                const unsigned g = std::min<unsigned>(nblk(m, HT), HEIII_SWEEP_BLOCKS);
                heiii_sweep_kernel<<<dim3(g), dim3(HT), sizeof(unsigned) * (size_t) L, s>>>(
                    m, E[cur], d_bub, L, p->BoxSize, tree_ready ? ctx->nodeB.ptr : nullptr, d_nfather, tree_ready ? ctx->pfather.ptr : nullptr, d_hit,
                    d_counts);
                SHQ_HIP(hipGetLastError());
                SHQ_TRY(sc.mark(s));
                SHQ_HIP(hipMemcpyAsync(counts.data(), d_counts, sizeof(unsigned long long) * (size_t) L, hipMemcpyDeviceToHost, s));
                SHQ_HIP(hipStreamSynchronize(s));
                st.ms[1] += sc.last_ms();
                st.ntests += (int64_t) m * L;
            }
            if(st.nsweeps < SHQ_HEIII_NSTAT) {
                st.sweep_draws[st.nsweeps] = (int32_t) draws.size();
                st.sweep_lit[st.nsweeps] = L;
                st.sweep_eligible[st.nsweeps] = m;
            }
            st.nsweeps++;
            st.ndraws += (int64_t) draws.size();
            st.nbubbles += L;
            /* ---- replay the loop's control (:530-590) over the batch */
            int k = 0, kstop = 0;
            for(const Draw &dr : draws) {
                const int64_t n_ionized = dr.cand >= 0 ? (int64_t) counts[(size_t) k++] : 0;
                kstop = k;
                curionfrac += (double) n_ionized / ngas;
                tot_n_ionized += n_ionized;
                if(log && iteration < log_capacity) {
                    shq_heiii_quasar &q = log[iteration];
                    memset(&q, 0, sizeof(q));
                    q.group = -1;
                    if(dr.cand >= 0) {
                        const CandRow &c = cand[(size_t) dr.cand];
                        q.group = (int32_t) c.group;
                        for(int d = 0; d < 3; d++) {
                            double x = c.cm[d] - p->CurrentParticleOffset[d];
                            if(isfinite(x)) {
                                while(x > p->BoxSize)
                                    x -= p->BoxSize;
                                while(x <= 0)
                                    x += p->BoxSize;
                            }
                            q.pos[d] = x;
                        }
                    }
                    q.ionfrac = curionfrac;
                    q.n_ionized = n_ionized;
                }
                const bool insufficient = n_ionized < 0.01 * non_overlapping_bubble_number && iteration > 10;
                iteration++;
                if(insufficient || !(curionfrac < p->desired_ion_frac)) {
                    stopped = true;
                    break;
                }
            }
            /* ---- flag and heat the particles whose first hit the loop reached; the rest stay eligible */
            SHQ_TRY(sc.mark(s));
            if(kstop > 0 && m > 0) {
                int64_t nsel = 0;
                SHQ_TRY(prim_partition_two_way(ctx, E[cur], rocprim::make_transform_iterator(d_hit, HitBefore{kstop}), S, E[cur ^ 1], (size_t) m, d_cnt, &nsel));
                if(nsel > 0) {
                    heiii_apply_rec_kernel<<<dim3(nblk(nsel, HT)), dim3(HT), 0, s>>>(nsel, S, d_flags, d_entropy, d_density, a3inv, du, d_rows + nrows);
                    SHQ_HIP(hipGetLastError());
                }
                nrows += nsel;
                m -= nsel;
                cur ^= 1;
            }
            SHQ_TRY(sc.mark(s));
            SHQ_HIP(hipEventSynchronize(sc.ev.back()));
            st.ms[2] += sc.last_ms();
            batch = std::min(2 * batch, HEIII_MAX_BATCH);
        }
        SHQ_CHECK(tot_n_ionized == nrows - result->n_flash, SHQ_ERR_STATE, "heiii: %ld particles counted, %ld flagged", (long) tot_n_ionized,
                  (long) (nrows - result->n_flash));
    }
    result->n_iterations = iteration;
    result->n_ionized = tot_n_ionized;
    result->final_ionfrac = curionfrac;
    if(nlog)
        *nlog = iteration;

    /* ---- the ionised rows into the caller's records: the flag bit alone (Generation, the time bins and Type share the word), Entropy */
    std::vector<double2> rows((size_t) std::max<int64_t>(nrows, 1));
    if(nrows > 0)
        SHQ_HIP(hipMemcpyAsync(rows.data(), d_rows, sizeof(double2) * (size_t) nrows, hipMemcpyDeviceToHost, s));
    SHQ_TRY(sc.mark(s));
    SHQ_HIP(hipStreamSynchronize(s));
    for(int64_t r = 0; r < nrows; r++) {
        const int64_t i = (int64_t) rows[(size_t) r].x;
        char *rec = static_cast<char *>(parts->base) + (size_t) i * parts->elsize;
        *reinterpret_cast<uint8_t *>(rec + parts->off_flags) |= (uint8_t) SHQ_FLAG_HEIII;
        const int32_t pi = *reinterpret_cast<const int32_t *>(rec + parts->off_pi);
        *reinterpret_cast<double *>(static_cast<char *>(sph->base) + (size_t) pi * sph->elsize + sph->off_entropy) = rows[(size_t) r].y;
    }
    st.ms[3] = sc.ms(0, sc.ev.size() - 1);
    ctx->heiii_stats = st;
    return SHQ_OK;
}
