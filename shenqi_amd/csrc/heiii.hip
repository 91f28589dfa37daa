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
 *
 * The same operator in phases (shq_heiii_open / _sweep / _commit / _close), for several ranks.  There every rank hosts some of the groups
 * and holds some of the gas, the hosting rank's walk reaches gas on every rank (treewalk export), and the loop's control needs each
 * bubble's count summed over the ranks.  So the run is cut where those sums are taken: open builds the eligible records (and returns
 * their extents, for the driver's culling), sweep records and counts first hits under the caller's numbering (seq), commit flags and
 * heats the records hit before a stop, close writes the rows back.  The run lives in the context (ctx->heiiirun); its buffers belong to
 * a CallScope that lives from open to close.  shq_heiii_reionization is a caller of the same steps (run_load, run_eligible, run_sweep,
 * run_commit, run_close): one sweep kernel, one apply kernel, one eligible-list builder, one row write-back.  Its bubbles are numbered
 * by their place among the lit ones of the batch, which is what the kernels recorded before there was a seq.
 * Across ranks membership must not depend on a rank's tree.  For R >= 0, +inf or NaN the particle test decides alone: cull_node never
 * rejects a node that holds a passing particle, and the top-tree export test (the same cull_node on the top nodes) is that argument
 * one level up.  For R < 0 (-inf: cull_node rejects the root, nothing is taken) the node tests decide too, so the phased sweep refuses
 * such a radius; the tree path stays with the one call.
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
    int32_t seq;     /* the number the bubble's hits are recorded and counted under: strictly increasing along the list */
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

/* one lane per eligible particle: the seq of the first lit bubble of the list that holds it (-1: none); the hits are counted per listed
 * bubble in LDS and flushed to counts[seq] */
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
            hit[i] = h >= 0 ? bub[h].seq : -1;
        }
        if(h >= 0)
            atomicAdd(&hist[h], 1u);
    }
    __syncthreads();
    for(int k = threadIdx.x; k < nb; k += HT)
        if(hist[k])
            atomicAdd(&counts[bub[k].seq], (unsigned long long) hist[k]);
}

/* per axis the smallest and largest coordinate of the records, in two passes: every workgroup reduces a grid-stride share to six
 * numbers, one workgroup reduces those.  min and max do not depend on the order they are taken in, so the result is the same bits on
 * every run.  No record: lo = +inf, hi = -inf.  fmin / fmax drop a NaN where numpy's min / max would carry it: the coordinates are
 * finite, because shq_particles_upload refuses a set with a non-finite position; extents of a resident set whose positions went
 * non-finite on the device are left undefined. */
__device__ __forceinline__ void extent_reduce(double v[6], double *out)
{
    __shared__ double sh[6][HT];
    for(int k = 0; k < 6; k++)
        sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for(int w = HT / 2; w > 0; w >>= 1) {
        if((int) threadIdx.x < w)
            for(int k = 0; k < 3; k++) {
                sh[k][threadIdx.x] = fmin(sh[k][threadIdx.x], sh[k][threadIdx.x + w]);
                sh[3 + k][threadIdx.x] = fmax(sh[3 + k][threadIdx.x], sh[3 + k][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if(threadIdx.x < 6)
        out[threadIdx.x] = sh[threadIdx.x][0];
}
__global__ __launch_bounds__(HT) void heiii_extent_kernel(long long m, const double4 *__restrict__ rec, double *__restrict__ part)
{
    const double inf = __builtin_huge_val();
    double v[6] = {inf, inf, inf, -inf, -inf, -inf};
    for(long long i = (long long) blockIdx.x * HT + threadIdx.x; i < m; i += (long long) gridDim.x * HT) {
        const double4 e = rec[i];
        v[0] = fmin(v[0], e.x), v[1] = fmin(v[1], e.y), v[2] = fmin(v[2], e.z);
        v[3] = fmax(v[3], e.x), v[4] = fmax(v[4], e.y), v[5] = fmax(v[5], e.z);
    }
    extent_reduce(v, part + 6 * (size_t) blockIdx.x);
}
__global__ __launch_bounds__(HT) void heiii_extent_final_kernel(int nparts, const double *__restrict__ part, double *__restrict__ out)
{
    const double inf = __builtin_huge_val();
    double v[6] = {inf, inf, inf, -inf, -inf, -inf};
    for(int i = threadIdx.x; i < nparts; i += HT)
        for(int k = 0; k < 3; k++) {
            v[k] = fmin(v[k], part[6 * (size_t) i + k]);
            v[3 + k] = fmax(v[3 + k], part[6 * (size_t) i + 3 + k]);
        }
    extent_reduce(v, out);
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

constexpr int HEIII_EXTENT_BLOCKS = 1024;

using Run = shq_context::HeiiiRun;

/* gaussian_rng(mean, sigma, MinID) (:249-255) */
double heiii_radius(double mean, double sigma, uint64_t minid, const double *rnd_table, int64_t rnd_size)
{
#pragma clang fp contract(off)
    const double u1 = rnd_table[minid % (uint64_t) rnd_size];
    const double u2 = rnd_table[(minid + 1) % (uint64_t) rnd_size];
    const double z1 = libm_sqrt(-2 * libm_log(u1)) * libm_cos(2 * M_PI * u2);
    return mean + sigma * z1;
}

double heiii_a3inv(const shq_heiii_params *p) { return 1 / libm_pow(p->atime, 3); }

/* non_overlapping_bubble_number (:514-518) */
int64_t heiii_bubble_threshold(const shq_heiii_params *p)
{
#pragma clang fp contract(off)
    const double rhobar = p->OmegaBaryon * (3 * HEIII_HUBBLE * p->HubbleParam * HEIII_HUBBLE * p->HubbleParam) / (8 * M_PI * HEIII_GRAVITY) * heiii_a3inv(p);
    const double totbubblegasmass = 4 * M_PI / 3. * libm_pow(p->mean_bubble, 3) * rhobar;
    return (int64_t) (p->n_gas_tot * totbubblegasmass / p->OmegaBaryon);
}

/* frees the run on the way out of a call that did not get as far as keeping it */
struct RunGuard {
    shq_context *ctx;
    bool keep = false;
    ~RunGuard()
    {
        if(!keep)
            shq_heiii_run_free(ctx);
    }
};

int run_check_inputs(const shq_heiii_params *p, const shq_part_view *parts, const shq_sph_view *sph)
{
    SHQ_CHECK(p->BoxSize > 0 && p->atime > 0 && p->n_gas_tot > 0, SHQ_ERR_INVALID, "heiii: BoxSize, atime and n_gas_tot must be > 0");
    SHQ_CHECK(parts->off_pos != SHQ_NOFIELD && parts->off_type != SHQ_NOFIELD && parts->off_flags != SHQ_NOFIELD && parts->off_pi != SHQ_NOFIELD,
              SHQ_ERR_INVALID, "heiii: the particle view needs Pos, Type, PI and the flag byte");
    SHQ_CHECK(sph->off_density != SHQ_NOFIELD && sph->off_entropy != SHQ_NOFIELD, SHQ_ERR_INVALID, "heiii: the gas view needs Density and Entropy");
    return SHQ_OK;
}

/* a run opens only on a context with no walk and no other run open */
int run_check_idle(shq_context *ctx)
{
    SHQ_CHECK(ctx->sphrun.phase == 0, SHQ_ERR_STATE, "heiii: an SPH walk is open");
    SHQ_CHECK(ctx->heiiirun.sc == nullptr, SHQ_ERR_STATE, "heiii: a HeIII run is open (shq_heiii_close first)");
    return SHQ_OK;
}

/* a new run: its scope, the first event, the counter words */
int run_begin(shq_context *ctx)
{
    Run &r = ctx->heiiirun;
    r = Run();
    r.sc = new CallScope(ctx, "heiii");
    SHQ_TRY(r.sc->mark(ctx->stream));
    SHQ_TRY(r.sc->alloc(&r.cnt, 2));
    return SHQ_OK;
}

/* particles and their gas state (uploaded, or the context's copies when the caller vouches for them), the flash (:501-512) and
 * gas_ionization_fraction's count (:330-346) */
int run_load(shq_context *ctx, const shq_heiii_params *p, const shq_part_view *parts, const shq_sph_view *sph, unsigned long long *nion_now)
{
#pragma clang fp contract(off)
    Run &r = ctx->heiiirun;
    CallScope &sc = *r.sc;
    hipStream_t s = ctx->stream;
    SHQ_TRY(shq_particles_upload(ctx, parts));
    SHQ_TRY(shq_sph_state_upload(ctx, parts, sph));
    const long long n = parts->numpart;
    r.n = n;
    r.box = p->BoxSize;
    r.a3inv = heiii_a3inv(p);
    const double nheperg = (1 - HEIII_HYDROGEN_MASSFRAC) / (HEIII_PROTONMASS * HEIII_HEMASS);
    const double deltau = p->qso_inst_heating * nheperg;
    r.du = deltau / p->uu_in_cgs;
    uint8_t *d_flags = ctx->pflags.ptr;
    SHQ_TRY(sc.alloc(&r.rows, (size_t) n)); /* (index, new Entropy) of every particle ionised by this run */
    if(p->desired_ion_frac > p->heIIIreion_finish_frac) {
        int32_t *fidx;
        SHQ_TRY(sc.alloc(&fidx, (size_t) n));
        int64_t nf = 0;
        SHQ_TRY(prim_select_if(ctx, rocprim::counting_iterator<int32_t>(0), fidx, (size_t) n, Flashable{d_flags}, r.cnt, &nf));
        if(nf > 0) {
            heiii_apply_idx_kernel<<<dim3(nblk(nf, HT)), dim3(HT), 0, s>>>(nf, fidx, d_flags, ctx->g_entropy.ptr, ctx->g_density.ptr, r.a3inv, r.du, r.rows);
            SHQ_HIP(hipGetLastError());
        }
        r.nrows = r.n_flash = nf;
    }
    SHQ_HIP(hipMemsetAsync(r.cnt, 0, sizeof(unsigned long long), s));
    if(n > 0) {
        heiii_count_kernel<<<dim3(nblk(n, HT)), dim3(HT), 0, s>>>(n, d_flags, r.cnt);
        SHQ_HIP(hipGetLastError());
    }
    SHQ_HIP(hipMemcpyAsync(nion_now, r.cnt, sizeof(*nion_now), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    return SHQ_OK;
}

/* the eligible gas, as records (x, y, z, index) the sweeps stream; the run is open from here on */
int run_eligible(shq_context *ctx)
{
    Run &r = ctx->heiiirun;
    CallScope &sc = *r.sc;
    int32_t *eidx;
    Bubble *bub;
    SHQ_TRY(sc.alloc(&eidx, (size_t) r.n));
    int64_t m = 0;
    SHQ_TRY(prim_select_if(ctx, rocprim::counting_iterator<int32_t>(0), eidx, (size_t) r.n, Eligible{ctx->pflags.ptr}, r.cnt, &m));
    SHQ_TRY(sc.alloc(&r.E[0], (size_t) m));
    SHQ_TRY(sc.alloc(&r.E[1], (size_t) m));
    SHQ_TRY(sc.alloc(&r.S, (size_t) m));
    SHQ_TRY(sc.alloc(&r.hit, (size_t) m));
    SHQ_TRY(sc.alloc(&bub, HEIII_MAX_BATCH));
    r.bub = bub;
    SHQ_TRY(sc.alloc(&r.counts, HEIII_MAX_BATCH));
    if(m > 0) {
        heiii_gather_kernel<<<dim3(nblk(m, HT)), dim3(HT), 0, ctx->stream>>>(m, eidx, ctx->posm.ptr, r.E[0]);
        SHQ_HIP(hipGetLastError());
    }
    r.m = r.st.neligible = m;
    r.cur = 0;
    r.phase = 1;
    return SHQ_OK;
}

int run_extents(shq_context *ctx, double lo[3], double hi[3])
{
    Run &r = ctx->heiiirun;
    hipStream_t s = ctx->stream;
    SHQ_TRY(r.sc->alloc(&r.ext, 6 * (size_t) (HEIII_EXTENT_BLOCKS + 1)));
    const int g = (int) std::min<unsigned>(nblk(r.m, HT), HEIII_EXTENT_BLOCKS);
    double *out = r.ext + 6 * (size_t) HEIII_EXTENT_BLOCKS;
    heiii_extent_kernel<<<dim3(g), dim3(HT), 0, s>>>(r.m, r.E[r.cur], r.ext);
    SHQ_HIP(hipGetLastError());
    heiii_extent_final_kernel<<<dim3(1), dim3(HT), 0, s>>>(g, r.ext, out);
    SHQ_HIP(hipGetLastError());
    double h[6];
    SHQ_HIP(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    for(int d = 0; d < 3; d++)
        lo[d] = h[d], hi[d] = h[3 + d];
    return SHQ_OK;
}

/* every phase after open: the run exists in the phase asked for, and the context still holds the particles it was opened on */
int run_check_phase(shq_context *ctx, int min_phase, const char *what)
{
    const Run &r = ctx->heiiirun;
    SHQ_CHECK(r.sc != nullptr && r.phase >= min_phase, SHQ_ERR_STATE, "heiii: %s out of order (phase %d)", what, r.sc ? r.phase : 0);
    SHQ_CHECK(ctx->have_parts && ctx->numpart == r.n, SHQ_ERR_STATE, "heiii: the context's particle set changed while the run was open");
    return SHQ_OK;
}

/* sweep the eligible records against L bubbles (seq strictly increasing, < nseq <= HEIII_MAX_BATCH); counts[nseq] on the host */
int run_sweep(shq_context *ctx, const Bubble *hb, int L, int nseq, const NodeB *nodeB, const int32_t *nfather, const int32_t *pfather,
              unsigned long long *counts)
{
    Run &r = ctx->heiiirun;
    CallScope &sc = *r.sc;
    hipStream_t s = ctx->stream;
    std::fill(counts, counts + nseq, 0ull);
    if(r.m > 0) { /* also with no bubble: every record's hit becomes -1, so a commit after it takes nothing */
        if(L > 0)
            SHQ_HIP(hipMemcpyAsync(r.bub, hb, sizeof(Bubble) * (size_t) L, hipMemcpyHostToDevice, s));
        SHQ_HIP(hipMemsetAsync(r.counts, 0, sizeof(unsigned long long) * (size_t) nseq, s));
        SHQ_TRY(sc.mark(s));
        const unsigned g = std::min<unsigned>(nblk(r.m, HT), HEIII_SWEEP_BLOCKS);
        heiii_sweep_kernel<<<dim3(g), dim3(HT), sizeof(unsigned) * (size_t) L, s>>>(r.m, r.E[r.cur], static_cast<const Bubble *>(r.bub), L, r.box, nodeB,
                                                                                  nfather, pfather, r.hit, r.counts);
        SHQ_HIP(hipGetLastError());
        SHQ_TRY(sc.mark(s));
        SHQ_HIP(hipMemcpyAsync(counts, r.counts, sizeof(unsigned long long) * (size_t) nseq, hipMemcpyDeviceToHost, s));
        SHQ_HIP(hipStreamSynchronize(s));
        r.st.ms[1] += sc.last_ms();
        r.st.ntests += r.m * L;
    }
    r.phase = 2;
    return SHQ_OK;
}

/* flag and heat the records whose first hit has seq < seq_stop; the rest stay eligible */
int run_commit(shq_context *ctx, int seq_stop, int64_t *n_committed)
{
    Run &r = ctx->heiiirun;
    CallScope &sc = *r.sc;
    hipStream_t s = ctx->stream;
    int64_t nsel = 0;
    SHQ_TRY(sc.mark(s));
    if(seq_stop > 0 && r.m > 0) {
        SHQ_TRY(prim_partition_two_way(ctx, r.E[r.cur], rocprim::make_transform_iterator(r.hit, HitBefore{seq_stop}), r.S, r.E[r.cur ^ 1], (size_t) r.m,
                                       r.cnt, &nsel));
        SHQ_CHECK(nsel >= 0 && r.nrows + nsel <= r.n, SHQ_ERR_STATE, "heiii: %ld rows for %ld particles", (long) (r.nrows + nsel), (long) r.n);
        if(nsel > 0) {
            heiii_apply_rec_kernel<<<dim3(nblk(nsel, HT)), dim3(HT), 0, s>>>(nsel, r.S, ctx->pflags.ptr, ctx->g_entropy.ptr, ctx->g_density.ptr, r.a3inv, r.du,
                                                                          r.rows + r.nrows);
            SHQ_HIP(hipGetLastError());
        }
        r.nrows += nsel;
        r.m -= nsel;
        r.cur ^= 1;
    }
    SHQ_TRY(sc.mark(s));
    SHQ_HIP(hipEventSynchronize(sc.ev.back()));
    r.st.ms[2] += sc.last_ms();
    r.phase = 1;
    *n_committed = nsel;
    return SHQ_OK;
}

/* the ionised rows into the caller's records: the flag bit alone (Generation, the time bins and Type share the word), Entropy.  The
 * run's statistics stay behind (ms[3]: the whole run from its first event, or the phases' times and this download), the run is freed. */
int run_close(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, bool whole)
{
    RunGuard guard{ctx};
    Run &r = ctx->heiiirun;
    CallScope &sc = *r.sc;
    hipStream_t s = ctx->stream;
    const int64_t nrows = r.nrows;
    std::vector<double2> rows((size_t) std::max<int64_t>(nrows, 1));
    SHQ_TRY(sc.mark(s));
    if(nrows > 0)
        SHQ_HIP(hipMemcpyAsync(rows.data(), r.rows, sizeof(double2) * (size_t) nrows, hipMemcpyDeviceToHost, s));
    SHQ_TRY(sc.mark(s));
    SHQ_HIP(hipStreamSynchronize(s));
    for(int64_t k = 0; k < nrows; k++) {
        const int64_t i = (int64_t) rows[(size_t) k].x;
        char *rec = static_cast<char *>(parts->base) + (size_t) i * parts->elsize;
        *reinterpret_cast<uint8_t *>(rec + parts->off_flags) |= (uint8_t) SHQ_FLAG_HEIII;
        const int32_t pi = *reinterpret_cast<const int32_t *>(rec + parts->off_pi);
        *reinterpret_cast<double *>(static_cast<char *>(sph->base) + (size_t) pi * sph->elsize + sph->off_entropy) = rows[(size_t) k].y;
    }
    r.st.ms[3] = whole ? sc.ms(0, sc.ev.size() - 1) : r.st.ms[0] + r.st.ms[1] + r.st.ms[2] + sc.last_ms();
    ctx->heiii_stats = r.st;
    return SHQ_OK;
}

} // namespace

void shq_heiii_run_free(shq_context *ctx)
{
    if(!ctx || !ctx->heiiirun.sc)
        return;
    delete ctx->heiiirun.sc; /* drains the stream, then frees the buffers and events */
    ctx->heiiirun = Run();
}

extern "C" int shq_heiii_last_stats(shq_context *ctx, shq_heiii_stats *stats)
{
    SHQ_CHECK(ctx && stats, SHQ_ERR_INVALID, "null argument");
    *stats = ctx->heiii_stats;
    return SHQ_OK;
}

extern "C" int shq_heiii_host_numbers(const shq_heiii_params *p, const uint64_t *minids, int64_t n, const double *rnd_table, int64_t rnd_size,
                                      double *radii_out, int64_t *non_overlapping_bubble_number)
{
    SHQ_CHECK(p && n >= 0 && (n == 0 || (minids && radii_out && rnd_table && rnd_size > 0)), SHQ_ERR_INVALID, "heiii_host_numbers: bad argument");
    const double sigma = libm_sqrt(p->var_bubble);
    for(int64_t i = 0; i < n; i++)
        radii_out[i] = heiii_radius(p->mean_bubble, sigma, minids[i], rnd_table, rnd_size);
    if(non_overlapping_bubble_number)
        *non_overlapping_bubble_number = heiii_bubble_threshold(p);
    return SHQ_OK;
}

extern "C" int shq_heiii_open(shq_context *ctx, const shq_heiii_params *p, const shq_part_view *parts, const shq_sph_view *sph, int64_t *n_flash,
                              int64_t *n_ionized_now, int64_t *n_eligible, double lo[3], double hi[3])
{
    SHQ_CHECK(ctx && p && parts && sph && n_flash && n_ionized_now && n_eligible && lo && hi, SHQ_ERR_INVALID, "heiii_open: null argument");
    SHQ_TRY(run_check_inputs(p, parts, sph));
    SHQ_TRY(run_check_idle(ctx));
    SHQ_HIP(hipSetDevice(ctx->device));
    RunGuard guard{ctx};
    SHQ_TRY(run_begin(ctx));
    Run &r = ctx->heiiirun;
    unsigned long long nion = 0;
    SHQ_TRY(run_load(ctx, p, parts, sph, &nion));
    SHQ_TRY(run_eligible(ctx));
    SHQ_TRY(run_extents(ctx, lo, hi));
    SHQ_TRY(r.sc->mark(ctx->stream));
    SHQ_HIP(hipEventSynchronize(r.sc->ev.back()));
    r.st.ms[0] = r.sc->ms(0, r.sc->ev.size() - 1);
    *n_flash = r.n_flash;
    *n_ionized_now = (int64_t) nion;
    *n_eligible = r.m;
    guard.keep = true;
    return SHQ_OK;
}

extern "C" int shq_heiii_sweep(shq_context *ctx, const shq_heiii_bubble *bubbles, int nbubbles, int nseq, uint64_t *counts)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx && counts && nbubbles >= 0 && (bubbles || nbubbles == 0), SHQ_ERR_INVALID, "heiii_sweep: bad argument");
    SHQ_TRY(run_check_phase(ctx, 1, "sweep"));
    SHQ_CHECK(nseq >= 1 && nseq <= HEIII_MAX_BATCH && nbubbles <= nseq, SHQ_ERR_INVALID, "heiii_sweep: nseq %d outside 1 .. %d, or %d bubbles for it",
              nseq, HEIII_MAX_BATCH, nbubbles);
    static_assert(HEIII_MAX_BATCH == SHQ_HEIII_MAX_SEQ, "the header's bound is the batch size");
    std::vector<Bubble> hb((size_t) nbubbles);
    for(int k = 0; k < nbubbles; k++) {
        const shq_heiii_bubble &in = bubbles[k];
        SHQ_CHECK(in.seq >= 0 && in.seq < nseq && (k == 0 || in.seq > bubbles[k - 1].seq), SHQ_ERR_INVALID,
                  "heiii_sweep: seq %d of bubble %d does not increase, or is outside 0 .. %d", in.seq, k, nseq - 1);
        /* a negative radius makes membership depend on the tree (cull_node), which differs from rank to rank */
        SHQ_CHECK(!(in.R < 0), SHQ_ERR_INVALID, "heiii_sweep: bubble %d has the negative radius %g", k, in.R);
        Bubble &b = hb[(size_t) k];
        memset(&b, 0, sizeof(b));
        for(int d = 0; d < 3; d++)
            b.c[d] = in.c[d];
        b.R = in.R;
        b.R2 = in.R * in.R;
        b.seq = in.seq;
    }
    SHQ_HIP(hipSetDevice(ctx->device));
    Run &r = ctx->heiiirun;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counts are 64-bit words");
    SHQ_TRY(run_sweep(ctx, hb.data(), nbubbles, nseq, nullptr, nullptr, nullptr, reinterpret_cast<unsigned long long *>(counts)));
    if(r.st.nsweeps < SHQ_HEIII_NSTAT) {
        r.st.sweep_lit[r.st.nsweeps] = nbubbles;
        r.st.sweep_eligible[r.st.nsweeps] = r.m;
    }
    r.st.nsweeps++;
    r.st.nbubbles += nbubbles;
    return SHQ_OK;
}

extern "C" int shq_heiii_commit(shq_context *ctx, int seq_stop, int64_t *n_committed)
{
    SHQ_CHECK(ctx && seq_stop >= 0 && seq_stop <= HEIII_MAX_BATCH, SHQ_ERR_INVALID, "heiii_commit: seq_stop %d outside 0 .. %d", seq_stop, HEIII_MAX_BATCH);
    SHQ_TRY(run_check_phase(ctx, 2, "commit"));
    SHQ_HIP(hipSetDevice(ctx->device));
    int64_t nsel = 0;
    SHQ_TRY(run_commit(ctx, seq_stop, &nsel));
    if(n_committed)
        *n_committed = nsel;
    return SHQ_OK;
}

extern "C" int shq_heiii_close(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, int64_t *n_rows)
{
    SHQ_CHECK(ctx && parts && sph, SHQ_ERR_INVALID, "heiii_close: null argument");
    SHQ_CHECK(ctx->heiiirun.sc != nullptr && ctx->heiiirun.phase >= 1, SHQ_ERR_STATE, "heiii: close without an open run");
    SHQ_CHECK(parts->numpart == ctx->heiiirun.n && parts->off_flags != SHQ_NOFIELD && parts->off_pi != SHQ_NOFIELD && sph->off_entropy != SHQ_NOFIELD,
              SHQ_ERR_INVALID, "heiii_close: not the records the run was opened on");
    SHQ_HIP(hipSetDevice(ctx->device));
    const int64_t nrows = ctx->heiiirun.nrows;
    SHQ_TRY(run_close(ctx, parts, sph, false));
    if(n_rows)
        *n_rows = nrows;
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
    SHQ_TRY(run_check_inputs(p, parts, sph));
    /* a negative radius makes membership depend on the tree (cull_node): a positive variance, or a negative mean, needs it */
    const bool need_tree = !(p->var_bubble <= 0) || p->mean_bubble < 0;
    SHQ_CHECK(!need_tree || (gas_tree && gas_tree->father), SHQ_ERR_INVALID, "heiii: var_bubble > 0 needs the gas tree with its father array");
    SHQ_CHECK(ctx->fof_ngroups >= 0, SHQ_ERR_STATE, "heiii: no FOF catalogue (run shq_fof first)");
    SHQ_TRY(run_check_idle(ctx));
    SHQ_HIP(hipSetDevice(ctx->device));
    memset(result, 0, sizeof(*result));
    if(nlog)
        *nlog = 0;
    hipStream_t s = ctx->stream;
    RunGuard guard{ctx}; /* the run never outlives this call */
    SHQ_TRY(run_begin(ctx));
    Run &r = ctx->heiiirun;
    CallScope &sc = *r.sc;
    shq_heiii_stats &st = r.st;

    /* ---- candidates, from the catalogue as it is now: a particle upload below drops it */
    const int64_t TotNgroups = ctx->fof_ngroups;
    std::vector<CandRow> cand;
    {
        int32_t *gidx;
        CandRow *rows;
        SHQ_TRY(sc.alloc(&gidx, (size_t) TotNgroups));
        int64_t K = 0;
        SHQ_TRY(prim_select_if(ctx, rocprim::counting_iterator<int32_t>(0), gidx, (size_t) TotNgroups,
                               InWindow{ctx->fof_groups.ptr, p->qso_candidate_min_mass, p->qso_candidate_max_mass}, r.cnt, &K));
        SHQ_TRY(sc.alloc(&rows, (size_t) K));
        if(K > 0) {
            heiii_cand_kernel<<<dim3(nblk(K, HT)), dim3(HT), 0, s>>>(K, gidx, ctx->fof_groups.ptr, rows);
            SHQ_HIP(hipGetLastError());
            cand.resize((size_t) K);
            SHQ_HIP(hipMemcpyAsync(cand.data(), rows, sizeof(CandRow) * (size_t) K, hipMemcpyDeviceToHost, s));
            SHQ_HIP(hipStreamSynchronize(s));
        }
    }

    /* ---- upload, flash ionisation (:501-512), gas_ionization_fraction (:330-346) and the bubble-count threshold (:514-518) */
    unsigned long long nion0 = 0;
    SHQ_TRY(run_load(ctx, p, parts, sph, &nion0));
    result->n_flash = r.n_flash;
    const double ngas = (double) p->n_gas_tot;
    const double initionfrac = (double) nion0 / ngas;
    double curionfrac = initionfrac;
    const int64_t non_overlapping_bubble_number = heiii_bubble_threshold(p);
    result->init_ionfrac = initionfrac;
    if(!(curionfrac < p->desired_ion_frac))
        cand.clear(); /* the candidate list is built only below the target */
    const int64_t K = (int64_t) cand.size();
    result->n_candidates = K;

    int64_t iteration = 0, tot_n_ionized = 0;
    if(K > 0) {
        SHQ_TRY(run_eligible(ctx));
        SHQ_TRY(sc.mark(s));
        SHQ_HIP(hipEventSynchronize(sc.ev.back()));
        st.ms[0] = sc.last_ms();
        int32_t *d_nfather = nullptr;
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
                    Bubble b;
                    memset(&b, 0, sizeof(b));
                    for(int k = 0; k < 3; k++)
                        b.c[k] = c.cm[k];
                    b.R = heiii_radius(p->mean_bubble, sigma, c.minid, rnd_table, rnd_size);
                    b.R2 = b.R * b.R;
                    b.neg = b.R < 0;
                    b.seq = (int32_t) hb.size(); /* the lit bubbles of the batch, numbered in list order */
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
            if(L > 0 && r.m > 0) {
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
                SHQ_TRY(run_sweep(ctx, hb.data(), L, L, tree_ready ? ctx->nodeB.ptr : nullptr, d_nfather, tree_ready ? ctx->pfather.ptr : nullptr,
                                  counts.data()));
            }
            if(st.nsweeps < SHQ_HEIII_NSTAT) {
                st.sweep_draws[st.nsweeps] = (int32_t) draws.size();
                st.sweep_lit[st.nsweeps] = L;
                st.sweep_eligible[st.nsweeps] = r.m;
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
            /* ---- flag and heat the particles whose first hit the loop reached; the rest stay eligible.  kstop > 0 only after a sweep
             * of this batch (a batch without lit bubbles leaves it 0), so the hits are this batch's */
            int64_t nsel = 0;
            SHQ_TRY(run_commit(ctx, r.m > 0 ? kstop : 0, &nsel));
            batch = std::min(2 * batch, HEIII_MAX_BATCH);
        }
        SHQ_CHECK(tot_n_ionized == r.nrows - r.n_flash, SHQ_ERR_STATE, "heiii: %ld particles counted, %ld flagged", (long) tot_n_ionized,
                  (long) (r.nrows - r.n_flash));
    }
    result->n_iterations = iteration;
    result->n_ionized = tot_n_ionized;
    result->final_ionfrac = curionfrac;
    if(nlog)
        *nlog = iteration;
    guard.keep = true; /* run_close frees it */
    return run_close(ctx, parts, sph, true);
}
