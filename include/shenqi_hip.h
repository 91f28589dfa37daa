/* shenqi_hip.h — C-ABI of the MI355X (gfx950) TreePM + SPH force engine.
 *
 * This is the drop-in boundary for shenqi's device seam: the four free functions the
 * reference calls when `UseGPU` is set,
 *     grav_short_tree_cuda   (libgadget/gravshort2.hpp:440-443, caller gravshort-tree2.cpp:151-154)
 *     density_cuda           (libgadget/densitytree2.hpp:437-439, caller density2.cpp:116-119)
 *     hydro_force_cuda       (libgadget/hydratree2.hpp:391-393,  caller hydra2.cpp:89-91)
 *     petapm_fft_r2c/_c2r + the host PM deposit/transfer/readout loops
 *                            (libgadget/petapm.h:136,143-144; petapm.cpp:392-465)
 * All entry points are extern "C", take plain pointers / sizes / POD structs and return an int
 * status (0 = ok).  On failure shq_last_error() returns a message; the shenqi-side shim turns
 * a non-zero status into endrun() (reference error convention: libgadget/utils/endrun.h:6,
 * device-launch check treewalk2.cuh:326-328).
 *
 * Ownership: the caller owns every host array; the library owns all device memory (its own
 * pools, never the caller's allocator: reference arena is LIFO, utils/memory.c).
 * Threading: one context per rank/GPU, calls come from the rank's main thread
 * (MPI_THREAD_FUNNELED, gadget/main.cpp:35).  Calls are synchronous unless stated.
 *
 * Two levels are offered:
 *   one-shot  (shq_grav_short_tree, shq_pm_force, shq_density, shq_hydro_force):
 *             host pointers in, host pointers out — what the reference call sites need;
 *   resident  (shq_particles_upload / shq_tree_upload / *_run / *_download):
 *             data stays in HBM between calls; used by time-step loops that keep particles
 *             on the device and by bench.py (timed region starts with inputs in HBM).
 */
#ifndef SHENQI_HIP_H
#define SHENQI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHQ_OK 0
#define SHQ_ERR_INVALID 1   /* bad argument / inconsistent view */
#define SHQ_ERR_DEVICE 2    /* HIP runtime / launch failure */
#define SHQ_ERR_NOMEM 3     /* device allocation failed */
#define SHQ_ERR_STATE 4     /* call order violated (e.g. run before upload) */
#define SHQ_ERR_NOCONV 5    /* Hsml iteration did not converge within MAXITER */

#define SHQ_NGRAVTAB 512    /* NGRAVTAB, libgadget/gravity.h:35 */
#define SHQ_NMAXCHILD 8     /* NMAXCHILD, libgadget/forcetree.h:13 */
#define SHQ_NODELISTLENGTH 4 /* NODELISTLENGTH, libgadget/localtreewalk2.h */
#define SHQ_TIMEBINS 46     /* TIMEBINS, libgadget/timebinmgr.h */

typedef struct shq_context shq_context;

/* ---- context ------------------------------------------------------------------------- */

/* Create a context on HIP device `device`.  `stream` is a hipStream_t to launch on (e.g.
 * torch's current stream) or NULL for a library-owned stream. */
int shq_init(int device, void *stream, shq_context **out);
void shq_shutdown(shq_context *ctx);
/* Last error message of the calling thread ("" if none). */
const char *shq_last_error(void);
/* Block until all work queued on the context's stream has finished. */
int shq_synchronize(shq_context *ctx);
/* The hipStream_t the context launches on (for event timing by the caller). */
void *shq_stream(shq_context *ctx);
/* HIP-event timer on the context's stream: begin/end bracket; elapsed returns ms of slot. */
int shq_timer_begin(shq_context *ctx, int slot);
int shq_timer_end(shq_context *ctx, int slot);
int shq_timer_elapsed_ms(shq_context *ctx, int slot, double *ms);
/* elapsed time between two recorded timer events (which: 0 begin, 1 end), e.g. the caller's slot 1 begin -> the library's walk (slot 19)
 * begin: where the phases of a resident step lie on one time line although they run on different streams.  Library slots: 8 PM begin,
 * 9 / 10 FFT pipeline begin / end, 13 PM end (all as begin events), 16 tree build, 19 tree walk.  The black-hole walks bracket their
 * device work as slots of their own (shq_timer_elapsed_ms): 15 walk + postprocess of shq_bh_accretion / shq_bh_feedback and of the emit pass
 * of shq_bh_accretion_marks / shq_bh_feedback_effects, or sort + kernel of shq_bh_marks_resolve / shq_bh_effects_apply; 17 the count pass;
 * 18 routing and sorting the emitted records. */
int shq_timer_between_ms(shq_context *ctx, int slot_a, int which_a, int slot_b, int which_b, double *ms);
/* Library version string. */
const char *shq_version(void);

/* ---- data views (reference layouts, no copies on the host side) ---------------------- */

/* Strided AoS view of `struct particle_data` (libgadget/partmanager.h:9-71), in the spirit of
 * PetaPMParticleStruct (libgadget/petapm.h:62-72): base pointer + element size + byte offsets.
 * An offset of SHQ_NOFIELD means "field not supplied". */
#define SHQ_NOFIELD ((size_t)-1)
typedef struct shq_part_view {
    void *base;             /* PartManager->Base */
    size_t elsize;          /* sizeof(struct particle_data) = 160 */
    int64_t numpart;        /* PartManager->NumPart */
    size_t off_pos;         /* double Pos[3] */
    size_t off_mass;        /* float  Mass */
    size_t off_type;        /* unsigned char Type */
    size_t off_flags;       /* unsigned int bitfield word: bit0 IsGarbage, bit1 Swallowed */
    size_t off_pi;          /* int PI (slot index) */
    size_t off_vel;         /* double Vel[3] */
    size_t off_treeacc;     /* double FullTreeGravAccel[3] */
    size_t off_gravpm;      /* double GravPM[3] */
    size_t off_potential;   /* double Potential */
    size_t off_hsml;        /* double Hsml */
    size_t off_dthsml;      /* double DtHsml */
    size_t off_timebin_hydro;   /* unsigned char TimeBinHydro */
    size_t off_timebin_gravity; /* unsigned char TimeBinGravity */
} shq_part_view;

/* Strided view of `struct sph_particle_data` (libgadget/slotsmanager.h:97-131), indexed by PI. */
typedef struct shq_sph_view {
    void *base;
    size_t elsize;          /* 176 */
    int64_t numslots;
    size_t off_density, off_egywtdensity, off_entropy, off_dtentropy, off_maxsignalvel;
    size_t off_hydroaccel;  /* double[3] */
    size_t off_dhsmlegydensityfactor, off_divvel, off_curlvel, off_delaytime;
} shq_sph_view;

/* Binary mirror of `struct NODE` (libgadget/forcetree.h:38-66), 120 bytes, so the host tree
 * (forcetree.cpp keeps ownership) is passed as-is. */
typedef struct shq_node {
    int32_t sibling;
    int32_t father;
    double len;
    double center[3];
    double cofm[3];     /* mom.cofm */
    double mass;        /* mom.mass */
    double hmax;        /* mom.hmax */
    int32_t suns[SHQ_NMAXCHILD];
    int32_t noccupied;
    uint32_t flags;     /* bit0 InternalTopLevel, bit1 TopLevel, bit2 DependsOnLocalMass, bits3-4 ChildType */
} shq_node;
#define SHQ_NODE_INTERNALTOPLEVEL(f) ((f) & 1u)
#define SHQ_NODE_TOPLEVEL(f) (((f) >> 1) & 1u)
#define SHQ_NODE_CHILDTYPE(f) (((f) >> 3) & 3u)
#define SHQ_PARTICLE_NODE_TYPE 0
#define SHQ_NODE_NODE_TYPE 1
#define SHQ_PSEUDO_NODE_TYPE 2

/* View of `ForceTree` (libgadget/forcetree.h:75-112). Index space as in the reference:
 * [0,firstnode) particles, [firstnode,firstnode+numnodes) nodes, >= lastnode pseudo. */
typedef struct shq_tree_view {
    const shq_node *nodes_base;  /* ForceTree.Nodes_base (Nodes = nodes_base - firstnode) */
    int64_t firstnode;
    int64_t lastnode;
    int64_t numnodes;
    int32_t rootnode;            /* node the primary walk starts from (== firstnode) */
    int32_t full_particle_tree_flag;
    double BoxSize;
    const int32_t *father;       /* ForceTree.Father (parent node of every particle) or NULL */
} shq_tree_view;

/* ---- short-range gravity -------------------------------------------------------------- */

/* POD mirror of GravTreeParams (libgadget/gravshort2.hpp:21-55) incl. GravShortTable
 * (libgadget/gravity.h:32-61) held by value exactly as the reference does. */
typedef struct shq_grav_params {
    double BoxSize;
    double cellsize;        /* BoxSize / Nmesh */
    double Rcut;            /* TreeParams.Rcut * Asmth * cellsize */
    double G;
    double cbrtrho0;
    double ForceSoftening;  /* FORCE_SOFTENING() = 2.8 * GravitySoftening */
    double ErrTolForceAcc;
    double BHOpeningAngle2; /* already squared; = MaxBHOpeningAngle^2 when TreeUseBH == 0 */
    int32_t TreeUseBH;
    int32_t pad_;
    float shortrange_table[SHQ_NGRAVTAB];
    float shortrange_table_potential[SHQ_NGRAVTAB];
    double dx;              /* table spacing in mesh cells */
} shq_grav_params;

typedef struct shq_walk_stats {
    int64_t ntargets;
    int64_t ninteractions;      /* sum over targets of the reference's visit() return value */
    int64_t min_interactions;
    int64_t max_interactions;
    int64_t nnodes_visited;     /* node tests executed by wavefronts (union walk) */
    int64_t nwave_interactions; /* interaction evaluations issued by wavefronts (x64 lanes each) */
    int64_t nwave_node_interactions; /* ... of which monopole (node) evaluations */
    int64_t nnode_interactions; /* per-target interactions that were node monopoles */
    double kernel_ms;           /* HIP-event time of the walk kernel(s) */
} shq_walk_stats;

/* Walk flavour.  Both reproduce the reference's per-target opening decisions and interaction set (interaction counts equal
 * the reference's as integers; parity bar runtests.cpp:441-443, SURVEY.md §8(c) rung L1).
 * EXACT: one target per lane, the wave walks the union of its 64 targets' walks depth-first; every target's contributions are
 *   summed in the reference's order.  Also serves the secondary (imported-query) walks.
 * GROUP: one SOURCE per lane; the wave takes its 64 targets as 8 groups of 8, every pending node carries the mask of the
 *   members whose own walk reaches it, node tests run 64 nodes at a time and each accepted source is applied to exactly the
 *   members that accept it.  Same interaction set per target, summed in a different order (forces agree to ~1e-15
 *   relative).  Measured at 256^3 (S-cluster): 73 ms against 39.5 ms for all particles, but 3.9 against 7.2 ms for every 64th and
 *   3.2 against 11.3 ms for every 512th particle of the same tree: the walk of choice for SPARSE active lists over a full tree.
 * AUTO: GROUP when an active list holds fewer than a tenth of the tree's particles (where the two lines above cross), EXACT
 *   otherwise — what the hierarchical integrator's levels should pass (timestep.cpp:437-446 walks ever shorter lists). */
#define SHQ_WALK_EXACT 0
#define SHQ_WALK_GROUP 1
#define SHQ_WALK_AUTO 2
/* flag, or-ed into walk_mode: with active == NULL, take the targets of the tree's particles sorted along a
 * Peano-Hilbert curve of their CURRENT positions (keys + radix sort on the device, ~2 ms for 1.7e7) instead of
 * particle-index order — same results per particle; keeps target groups compact when the particle
 * order has gone stale (resident stepping without the reference's periodic Peano-Hilbert re-sort) */
#define SHQ_WALK_TREE_ORDER 0x100
/* flag, or-ed into walk_mode: leave the raw sums of the primary walk on the device and skip
 * GravTreeOutput::postprocess; shq_grav_reduce_export_results then adds the results of the exported queries
 * (ev_reduce_export_result, treewalk2.h:793-812) and shq_grav_postprocess finishes (ev_postprocess, :375-382) —
 * the order the reference's distributed walk keeps. */
#define SHQ_WALK_DEFER_POSTPROCESS 0x200

/* Order of n device-resident positions (rows of 4 doubles: x, y, z, anything) along the Peano-Hilbert curve the walk groups its
 * targets by (the order SHQ_WALK_TREE_ORDER walks in): d_order[k] = row index of the k-th particle, equal keys in index order.
 * What a driver calls after a domain exchange in place of the reference's particle sort (domain.cpp:268, slots_gc_sorted), without
 * bringing the positions to the host.  Both pointers are device pointers; the work is queued on the context's stream. */
int shq_hilbert_order(shq_context *ctx, const double *d_posm, int64_t n, double BoxSize, int64_t *d_order);

/* One-shot replacement of grav_short_tree_cuda(): walks the local tree for the `nactive`
 * targets in `active` (NULL => all particles, as ActiveParticles with a NULL list), writes
 * Accel[target][0..2] (already multiplied by G: GravTreeOutput::postprocess,
 * gravshort2.hpp:88-107) and, when update_potential, also FullTreeGravAccel and Potential
 * inside the particle view. `accel` is indexed by particle index, numpart rows. */
int shq_grav_short_tree(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts,
                        const int32_t *active, int64_t nactive, const shq_grav_params *params,
                        double (*accel)[3], int update_potential, int walk_mode,
                        shq_walk_stats *stats);

/* Resident API. */
int shq_particles_upload(shq_context *ctx, const shq_part_view *parts);
/* One-shot operators upload the views they are handed — particles, SPH state, tree, and the ID array of the sub-grid walks: at 2 x 10^6
 * particles 50-170 ms of packing and PCIe around 4-7 ms of kernels, and run.cpp:621-681 calls a handful of them per step on the same
 * particles.  With a bit of `mask` set the caller vouches that the context's copy of that input IS the view it passes next: same base
 * pointer and count, contents unchanged on the host since the copy was made or changed only by the library's own operators (which
 * write what they change to the views and to the context alike; shq_metal_return, which changes masses and densities in the caller's
 * records only, takes the particle and SPH bits back itself).  Those uploads are then skipped.  A drift, a kick, a device-side particle
 * hand-over or mask = 0 ends it. */
#define SHQ_CURRENT_PARTICLES 1
#define SHQ_CURRENT_SPH 2
#define SHQ_CURRENT_TREE 4
#define SHQ_CURRENT_IDS 8
int shq_set_inputs_current(shq_context *ctx, int mask);

int shq_tree_upload(shq_context *ctx, const shq_tree_view *tree);

/* Device tree build.  Replaces, for a single-domain tree, force_tree_rebuild / force_tree_create_nodes
 * (libgadget/forcetree.cpp:727-859), force_tree_calc_moments / force_update_node_parallel (:1016-1142)
 * and the host repack + H2D of shq_tree_upload: builds the oct-tree of the uploaded particles whose type
 * is in `mask` (bit t = particle type t; garbage and swallowed particles are skipped, as in
 * forcetree.cpp:692-705), optionally restricted to the `active` list (host pointer, ActiveParticles
 * order), computes mass / centre of mass / hmax and installs it as the context's current tree.
 * The tree is the one the reference's insertion build produces for the same particles (same cells,
 * same leaves in the same particle order, same moments to the bit).  Returns SHQ_ERR_INVALID when more
 * than 8 particles lie within Box/2^21 of each other (deeper than the device build supports): the caller
 * then keeps its host build; nothing is truncated. */
typedef struct shq_tree_build_stats {
    int64_t nparticles;   /* particles in the tree */
    int64_t numnodes;
    int32_t maxdepth;
    float build_ms;       /* device time, HIP events */
} shq_tree_build_stats;
int shq_tree_build(shq_context *ctx, double BoxSize, int mask, const int32_t *active, int64_t nactive,
                   shq_tree_build_stats *stats);
/* The device-built tree in the reference's format (struct NODE, forcetree.h:38-66): `nodes[k]` is node
 * number firstnode + k (pre-order, root first), links (sibling, father, suns of internal nodes) are node
 * numbers, leaf suns are particle indices; `father[i]` = node number of the leaf holding particle i or
 * -1 (ForceTree.Father).  Either output may be NULL; *numnodes always returns the node count.  After shq_tree_build_domain the
 * top-level nodes carry TopLevel / InternalTopLevel and pseudo nodes suns[0] = firstnode + capacity + leaf (lastnode is the end of
 * the caller's node array). */
int shq_tree_download(shq_context *ctx, int64_t firstnode, shq_node *nodes, int64_t capacity, int32_t *father,
                      int64_t *numnodes);

/* Device tree build under a domain decomposition: the top-tree and pseudo-particle part of force_tree_create_nodes
 * (force_tree_create_topnodes / force_create_node_for_topnode, libgadget/forcetree.cpp:651-690, 868-930), the moments of the
 * local sub-trees, and force_exchange_pseudodata / force_treeupdate_pseudos (:1136-1281) around the caller's all-gather.
 *
 * The top tree arrives as geometry: for every TopNode its eight daughters in octant order `count = i + 2 j + 4 k`
 * (the slot force_create_node_for_topnode puts TopNodes[Daughter + sub] in, sub = 7 & peano_hilbert_key(2x + i, 2y + j, 2z + k,
 * bits) — the reference-side shim fills the table with its own key function, INTEGRATION.md, or takes it from shq_domain_install),
 * -1 eight times for a leaf, and the leaf's TopLeaves index.  topleaves[].Task says whose each leaf is.
 *
 * shq_tree_build_domain: as shq_tree_build, but every TopNode is a tree node whether or not it holds particles (empty top-level
 * nodes are never removed, forcetree.cpp:1040-1045), a leaf of ThisTask roots an ordinary sub-tree of this rank's particles, a
 * leaf of another task is a pseudo node (ChildType PSEUDO, suns[0] = lastnode + leaf).  SHQ_ERR_INVALID if a particle of the
 * list lies in a leaf of another task (the reference ends the run: "Bad topleaf").  Outputs: topleaves[].treenode = firstnode +
 * pre-order number of the leaf's node (what shq_tree_download numbers it), local_moments[leaf] = {s, mass, hmax} of the leaves
 * of ThisTask (zero elsewhere): the caller's contribution to the all-gather of force_exchange_pseudodata.
 * shq_tree_set_topleaf_moments: after the all-gather; the moments of the other tasks' leaves go into their pseudo nodes, the
 * internal top-level nodes are re-summed over their eight daughters (force_treeupdate_pseudos) and the top tree is installed for
 * shq_grav_toptree_exports / shq_ngb_toptree_exports (no shq_toptree_upload needed).  A one-task domain needs no second call. */
typedef struct shq_topleaf {   /* struct topleaf_data, libgadget/domain.h:20-24 */
    int32_t Task;
    int32_t topnode;
    int32_t treenode;
} shq_topleaf;
typedef struct shq_topnode_geo {
    int32_t daughter[8];    /* TopNodes index per octant, all -1 for a leaf */
    int32_t leaf;           /* TopLeaves index of a leaf, -1 otherwise */
    int32_t pad_;
} shq_topnode_geo;
typedef struct shq_topleaf_moments {   /* struct topleaf_momentsdata, forcetree.cpp:1129-1134 */
    double s[3];
    double mass;
    double hmax;
} shq_topleaf_moments;
int shq_tree_build_domain(shq_context *ctx, double BoxSize, int mask, const int32_t *active, int64_t nactive,
                          const shq_topnode_geo *topnodes, int ntopnodes, shq_topleaf *topleaves, int ntopleaves, int ThisTask,
                          int64_t firstnode, shq_topleaf_moments *local_moments, shq_tree_build_stats *stats);
int shq_tree_set_topleaf_moments(shq_context *ctx, const shq_topleaf_moments *moments, int ntopleaves);
/* The particle loop of domain_maintain() (libgadget/domain.cpp:296-330, 347-368) after shq_drift, on the domain of the last
 * shq_tree_build_domain (its top tree and the cells of its top-level nodes): a live particle that is still inside the cell of its
 * top leaf keeps it (inside_topleaf, bounds included), any other gets TopLeaf = domain_get_topleaf(PEANO(Pos)) (domain.h:68-76,
 * utils/peano.h:15-21: the descent through the daughter table on PEANO()'s integer coordinates finds the same leaf); d_target
 * (may be NULL) = layoutfunc: the leaf's task, -1 for garbage and, when dmtree == 0, for dark matter whose gravity bin is not
 * active at Ti_Current (it stays and keeps its leaf).  d_topleaf / d_target are DEVICE arrays of one int per resident particle —
 * d_target is what shq_exchange_plan takes.  *nchanged = particles that left their leaf. */
int shq_domain_maintain_topleaf(shq_context *ctx, int dmtree, int64_t Ti_Current, int32_t *d_topleaf, int32_t *d_target, int64_t *nchanged);

/* ---- the domain decomposition itself (domain_decompose_full, libgadget/domain.cpp:174-277) -----------------------------------------
 * The particle loops run on the device, the small serial stages are host functions of the library, the collectives between them are
 * the caller's (shenqi_amd/dist.py: DistDomain).  Every result is integers; nothing here has a tolerance.
 *
 * The reference's key, PEANO() (utils/peano.h:15-21), is a finite automaton over the octants of a position, most significant bit
 * first: key digit = sub[state][octant], state' = next[state][octant], octant = (xbit << 2) | (ybit << 1) | zbit, state 0 at the root.
 * The library holds no table of its own: shq_peano_tables_from_key recovers the automaton from a key function the caller hands it
 * (the reference-side shim passes peano_hilbert_key).  Two octant paths are the same state when the low digits of the keys of all
 * their two-level continuations agree; the walk from the root closes at 24 states for the reference's curve.  SHQ_ERR_INVALID when
 * more than SHQ_PEANO_MAXSTATES states appear or when the tables do not reproduce keyfn(x, y, z, 21) on 4096 pseudo-random triples
 * (the function is no such automaton).  shq_peano_tables is plain data: a caller may store and reload it. */
#define SHQ_PEANO_MAXSTATES 64
#define SHQ_PEANO_BITS 21                    /* BITS_PER_DIMENSION */
#define SHQ_PEANOCELLS (1ull << 63)          /* PEANOCELLS: the key of a garbage sample */
#define SHQ_ERR_RETRY 6     /* the top tree does not fit MaxTopNodes: nothing was written, call again with more ("retry", domain.cpp:199-214) */
typedef uint64_t (*shq_peano_keyfn)(int x, int y, int z, int bits);
typedef struct shq_peano_tables {
    int32_t nstates;
    uint8_t next[SHQ_PEANO_MAXSTATES][8];
    uint8_t sub[SHQ_PEANO_MAXSTATES][8];
} shq_peano_tables;
int shq_peano_tables_from_key(shq_peano_keyfn keyfn, shq_peano_tables *out);
/* peano_hilbert_key(x, y, z, bits) from the tables, on the host (1 <= bits <= 21): what the device kernels compute */
uint64_t shq_peano_key_host(const shq_peano_tables *tables, int x, int y, int z, int bits);
/* d_keys[i] = PEANO(pos_i, BoxSize), bit for bit: the same three double operations and truncation to int, then the automaton.
 * pos_i = the three doubles at d_pos + i * stride_bytes (24 for a packed array, the record size for Pos inside particle_data).
 * d_keys is what shq_slots_gc_sorted takes.  One particle per lane; the tables sit in LDS, two levels per lookup. */
int shq_peano_keys(shq_context *ctx, const shq_peano_tables *tables, const void *d_pos, size_t stride_bytes, int64_t n, double BoxSize, uint64_t *d_keys);

/* A device-readable particle_data array as shq_exchange_* take it (bit 0 of the byte at off_flags = IsGarbage), plus Pos. */
typedef struct shq_domain_parts {
    const void *d_parts;
    size_t elsize, off_flags, off_pos;
    int64_t numpart;
    double BoxSize;
} shq_domain_parts;
/* The subsample of domain_check_for_local_refine_subsample (domain.cpp:1005-1067).  PreSort == 0: the keys of every
 * SubSampleDistance-th slot (one sample when NumPart is below the distance), garbage samples dropped.  PreSort != 0: all keys, garbage
 * as PEANOCELLS, sorted, then every SubSampleDistance-th of the live ones (one when fewer live than the distance).  d_samples (device,
 * room for NumPart / SubSampleDistance + 1 keys) comes out sorted; *nsample = their number.  The sort across ranks is the caller's. */
int shq_domain_samples(shq_context *ctx, const shq_peano_tables *tables, const shq_domain_parts *parts, int SubSampleDistance, int PreSort,
                       uint64_t *d_samples, int64_t *nsample);
/* The local top tree of sorted samples (domain.cpp:1073-1168, then domain_toptree_truncate :892-958), numbered as the reference's
 * serial loop numbers it (the closed form of the skeleton).  Every sample counts and costs 1.  tree (host, MaxTopNodes
 * entries) receives the nodes that survive the truncation, *size their number.  SHQ_ERR_RETRY when the skeleton before truncation has
 * more than MaxTopNodes nodes (domain_toptree_split's "ran out of top nodes"): tree and *size are not written.  nsample == 0 gives the
 * root alone. */
typedef struct shq_local_topnode {   /* struct local_topnode_data, domain.cpp:60-70 */
    uint64_t StartKey;
    int32_t Shift;
    int32_t Daughter;
    int32_t Parent;
    int32_t pad_;
    int64_t Count;
    int64_t Cost;
} shq_local_topnode;
int shq_domain_local_toptree(shq_context *ctx, const uint64_t *d_sorted_samples, int64_t nsample, int64_t countlimit, int64_t costlimit, int MaxTopNodes,
                             shq_local_topnode *tree, int *size);
/* The serial stages, pure host code (no context):
 *   shq_domain_toptree_merge   domain_toptree_merge (:1447-1552) of treeB into treeA from the two roots.  Where the reference ends
 *                              the run (no room for eight more nodes, a corrupt treeB) this returns SHQ_ERR_RETRY / SHQ_ERR_INVALID;
 *                              treeA is then partly merged and must be discarded.
 *   shq_domain_toptree_finish  domain_global_refine (:1320-1371; SHQ_ERR_RETRY when out of nodes), the copy into TopNodes (:469-476)
 *                              and domain_create_topleaves (:801-816).  TopNodes / TopLeaves have room for MaxTopNodes entries.
 *   shq_domain_balance         domain_assign_topleaves_balanced (:619-761, one segment per task, the sentinel entry TopLeaves[ntopleaves]
 *                              = {NTask, -1} included: TopLeaves has room for ntopleaves + 1), domain_set_task_leafs (:764-793, Tasks
 *                              has NTask + 1 entries) and domain_check_memory_bound (:529-585): *status = 1 when the largest load
 *                              exceeds MaxPart * SetAsideFactor.  As in the reference the loads are summed over TopLeafCount[StartLeaf
 *                              .. EndLeaf), the counts in their order before the assignment.  SHQ_ERR_INVALID where the reference
 *                              ends the run (fewer leaves than tasks, not enough segments). */
typedef struct shq_topnode {   /* struct topnode_data, libgadget/domain.h:12-18 */
    uint64_t StartKey;
    int32_t Daughter;
    int32_t Shift;
    int32_t Leaf;
    int32_t pad_;
} shq_topnode;
typedef struct shq_task_leafs { /* struct task_data, domain.h:26-29 */
    int32_t StartLeaf;
    int32_t EndLeaf;
} shq_task_leafs;
int shq_domain_toptree_merge(shq_local_topnode *treeA, int *sizeA, const shq_local_topnode *treeB, int sizeB, int MaxTopNodes);
int shq_domain_toptree_finish(shq_local_topnode *tree, int *size, int MaxTopNodes, int64_t countlimit, int64_t costlimit, shq_topnode *TopNodes,
                              shq_topleaf *TopLeaves, int *ntopleaves);
int shq_domain_balance(shq_topnode *TopNodes, int ntopnodes, shq_topleaf *TopLeaves, int ntopleaves, const int64_t *TopLeafCount, int NTask,
                       int64_t MaxPart, double SetAsideFactor, shq_task_leafs *Tasks, int *status);
/* Makes a decomposition the context's current one: uploads the key-space tree (what shq_domain_leaf_counts and
 * shq_domain_particle_topleaves descend) and fills geo_out (may be NULL; ntopnodes entries), the daughter-per-octant table
 * shq_tree_build_domain takes: a node's state follows `next` from its parent's, daughter[i + 2 j + 4 k] = Daughter +
 * sub[state][(i << 2) | (j << 1) | k].  SHQ_ERR_INVALID for a tree that is none (a Daughter that does not lie behind its node, a leaf
 * without a valid Leaf, an internal node with Shift < 3). */
int shq_domain_install(shq_context *ctx, const shq_peano_tables *tables, const shq_topnode *TopNodes, int ntopnodes, const shq_topleaf *TopLeaves,
                       int ntopleaves, shq_topnode_geo *geo_out);
/* domain_compute_costs (:1374-1429, counts only) before its all-reduce: TopLeafCount[leaf] (host, ntopleaves entries) = live particles
 * whose domain_get_topleaf(PEANO(Pos)) (domain.h:69-76) is that leaf, on the installed tree. */
int shq_domain_leaf_counts(shq_context *ctx, const shq_domain_parts *parts, int64_t *TopLeafCount);
/* The loop of domain.cpp:238-246 and DomainExchangePlan::layoutfunc (:159-164) on the installed tree: d_topleaf[i] = the top leaf of
 * every live particle, d_target[i] (may be NULL) = that leaf's Task: what shq_exchange_plan takes.  Garbage keeps its old leaf and
 * gets target -1, as in shq_domain_maintain_topleaf. */
int shq_domain_particle_topleaves(shq_context *ctx, const shq_domain_parts *parts, int32_t *d_topleaf, int32_t *d_target);

/* Resident drift and kick: with the particles, their velocities and the force
 * arrays in HBM a step is  shq_drift -> shq_tree_build -> shq_pm_run / shq_grav_short_run -> kicks,
 * without a PCIe crossing.  Same operations in the same order as the reference, so the state stays
 * bit-identical to a host integration.  Black-hole repositioning (drift.cpp:32-53) and the black-hole part of
 * do_hydro_kick need the BH slot fields (shq_bh_dynamics_upload below); the particle loops of the integer time line are
 * shq_find_timesteps and its relatives below, DriftKickTimes and the sync points stay with the host.
 *
 * shq_dynamics_upload: Vel, Hsml, DtHsml, TimeBinGravity of the particles uploaded before.
 * shq_drift: drift_all_particles / real_drift_particle (libgadget/drift.cpp:16-99):
 *     Pos += Vel * ddrift + random_shift, wrapped into (0, BoxSize]; gas Hsml += DtHsml * ddrift, capped at
 *     BoxSize / 2; garbage / swallowed particles only follow the shift.  Invalidates the tree and the PM result.
 *     SHQ_ERR_INVALID for a non-finite position or a gas Hsml <= 0 (the reference ends the run).
 * shq_kick_short: apply_half_kick, gravity part (timestep.cpp:838-872, 962-968):
 *     Vel += A * gravkick[TimeBinGravity] for the active list (NULL => all), A = FullTreeGravAccel, or the
 *     walk's Accel output (AccelStore, timestep.cpp:273) when from_accel_store; inactive bins carry 0.
 * shq_kick_pm: apply_PM_half_kick (timestep.cpp:937-959): Vel += GravPM * Fgravkick for every particle.
 * shq_dynamics_download: Pos, Vel, Hsml back into the caller's particle array. */
int shq_dynamics_upload(shq_context *ctx, const shq_part_view *parts);

/* Active-particle lists on the device (build_active_particles / build_active_sublist,
 * libgadget/timestep.cpp:1286-1390).  The lists stay in HBM; SHQ_ACTIVE_RESIDENT / SHQ_SUBLIST_RESIDENT passed as
 * the `active` argument of shq_tree_build, shq_grav_short_run and shq_kick_short select them (nactive is ignored),
 * so a sub-step of the hierarchical integrator never moves an index list over PCIe.
 *
 * shq_timebins_upload: TimeBinGravity / TimeBinHydro of the resident particles (host arrays of numpart bytes;
 *     NULL keeps what is there, zero if nothing is).  shq_dynamics_upload and shq_sph_upload also set them.
 * shq_build_active_particles: ActivePredicate (timestep.cpp:1265-1282) over all particles, in index order (std::copy_if
 *     is stable): not garbage / swallowed, and gravity bin active or (gas / BH and hydro bin active) at Ti_Current
 *     (is_timebin_active, timestep.cpp:132-139).  is_pm_step: the reference's PM-step branch, every particle is active
 *     and ActiveParticle stays NULL (NumActiveHydro then counts the type-0/5 records, where the reference reports its
 *     slot-array sizes).  info may be NULL.
 * shq_build_active_sublist: SubActivePredicate (timestep.cpp:1354-1371) over the resident list: gravity bin <= maxtimebin
 *     and active.
 * shq_active_download: either list to the host (count always returned; list may be NULL). */
typedef struct shq_active_info {
    int64_t NumActiveParticle, NumActiveGravity, NumActiveHydro;
    int64_t TimeBinCountType[6 * (SHQ_TIMEBINS + 1)];   /* [(TIMEBINS + 1) * type + bin] */
} shq_active_info;
#define SHQ_ACTIVE_RESIDENT ((const int32_t *) (intptr_t) -1)
#define SHQ_SUBLIST_RESIDENT ((const int32_t *) (intptr_t) -2)
#define SHQ_SPH_QUEUE_RESIDENT ((const int32_t *) (intptr_t) -3)   /* the current work queue of an open SPH walk */
int shq_timebins_upload(shq_context *ctx, const uint8_t *bin_gravity, const uint8_t *bin_hydro);
int shq_build_active_particles(shq_context *ctx, int64_t Ti_Current, int is_pm_step, shq_active_info *info);
int shq_build_active_sublist(shq_context *ctx, int maxtimebin, int64_t Ti_Current, int64_t *nsub);
int shq_active_download(shq_context *ctx, int sublist, int32_t *list, int64_t capacity, int64_t *count);
int shq_drift(shq_context *ctx, double ddrift, double BoxSize, const double random_shift[3]);
int shq_kick_short(shq_context *ctx, const double gravkick[SHQ_TIMEBINS + 1], const int32_t *active, int64_t nactive,
                   int from_accel_store);
int shq_kick_pm(shq_context *ctx, double Fgravkick);
/* do_hydro_kick for gas (timestep.cpp:970-1003) as apply_half_kick / apply_hydro_half_kick call it (:875-886, :914-934):
 * Vel += HydroAccel * hydrokick[TimeBinHydro], the MaxGasVel clamp (|Vel| / atime <= MaxGasVel; *nlimited counts the
 * clamped particles, which the reference logs), Entropy += DtEntropy * dt_entr[TimeBinHydro] — on the SPH state the last
 * shq_density / shq_hydro_force (or phase calls) left resident; from_hydro_output takes HydroAccel / DtEntropy from that
 * hydro run instead of the uploaded SphP values.  Inactive bins carry 0 in both tables.  The black-hole part (DFAccel,
 * DragAccel) needs the BH slot arrays and stays with the host.  shq_entropy_download: Entropy by particle index. */
int shq_kick_hydro(shq_context *ctx, const double hydrokick[SHQ_TIMEBINS + 1], const double dt_entr[SHQ_TIMEBINS + 1], double atime,
                   double MaxGasVel, const int32_t *active, int64_t nactive, int from_hydro_output, int64_t *nlimited);
int shq_entropy_download(shq_context *ctx, double *entropy_by_particle);
int shq_dynamics_download(shq_context *ctx, const shq_part_view *parts);

/* The integer time line on the device (libgadget/timestep.cpp:157-194, 307-446, 584-822, 1012-1110):
 * new time bins for the resident particles from the accelerations, smoothing lengths and signal velocities that are in HBM
 * already.  The sync-point table, the cosmology and DriftKickTimes stay with the host (integration/reference_side/timestep.cpp mirrors
 * find_timesteps / find_hydro_timesteps / hierarchical_gravity_and_timesteps over these calls); the per-particle loops and
 * their reductions run here.  IEEE sqrt and divide, no fma contraction: the bins equal the host loop's as integers.
 *
 * shq_timeline: what TimeBinMgr::dti_from_dloga and get_dloga_for_bin read at Ti_Current (timebinmgr.h:120-176, 228-243):
 *     loga_now = SyncPoints[lastsnap].loga + (Ti_Current & (TIMEBASE - 1)) * Dloga_interval; the segment the step starts in
 *     (seg_snap[0], lower sync point index after the reference's clamps) with its two ends seg_loga[0..1], and when a further
 *     sync point exists (nseg = 2) the one after, seg_snap[1] = seg_snap[0] + 1, ending at seg_loga[2]. */
typedef struct shq_timeline {
    int64_t Ti_Current;
    double loga_now;
    double Dloga_interval;      /* Dloga_interval_ti(Ti_Current), 0 past the last sync point */
    int32_t nseg;
    int32_t pad_;
    int64_t seg_snap[2];
    double seg_loga[3];
} shq_timeline;

/* TimestepParams (timestep.cpp:35-50) and the arguments of the loops.  fac3 = pow(atime, 3 (1 - GAMMA) / 2) (timestep.cpp:1049),
 * ForceSoftening = FORCE_SOFTENING(), dti_max = times->PM_length after the PM-step update of the caller. */
typedef struct shq_timestep_params {
    double ErrTolIntAccuracy, CourantFac, MinSizeTimestep;
    double ForceSoftening;
    double atime, hubble, fac3;
    int64_t dti_max;
    int32_t ForceEqualTimesteps;
    int32_t isFirstTimeStep;
    int32_t mintimebin, mingravtimebin;   /* times->mintimebin / mingravtimebin on entry (find_hydro_timesteps reads them) */
    shq_timeline tl;
} shq_timestep_params;

typedef struct shq_timestep_result {
    int32_t badstepsizecount;
    int32_t mTimeBin, maxTimeBin;         /* min / max new bin over the list (TIMEBINS / 0 when the list is empty) */
    int32_t mintimebin;                   /* find_hydro_timesteps: times->mintimebin after its fix-ups (timestep.cpp:677-696) */
    int64_t ntiaccel, nticourant, ntihsml, ntiaccrete, ntineighbour;
    int64_t nbh, dynratio;                /* find_hydro_timesteps: BHs on the list, sum of TimeBinDynFric - TimeBinHydro */
    int32_t maxdyndiff;
    int32_t nbadbin;                      /* particles the reference would print_bad_timebin for */
    int64_t dti_min;                      /* ForceEqualTimesteps: find_global_timestep (before the caller's MPI minimum) */
    int64_t timebincounts[SHQ_TIMEBINS + 1]; /* shq_hier_gravity_bins */
} shq_timestep_result;

/* find_timesteps particle loop (timestep.cpp:733-792): new TimeBinHydro = TimeBinGravity for the list (NULL: all; the
 * resident lists are accepted) from the gravity criterion on FullTreeGravAccel + GravPM and, for gas / BH, the hydro criteria
 * (MaxSignalVel of the last hydro run or upload, Hsml, DtHsml; the BH neighbour limiter needs shq_bh_dynamics_upload).
 * ForceEqualTimesteps: dti_min_global (the caller's reduction of shq_find_global_timestep over ranks) is every particle's step.
 * isFirstTimeStep: set_bh_first_timestep(mTimeBin) with mTimeBin_global >= 0, otherwise with this list's own minimum.
 * The caller applies the DriftKickTimes updates of timestep.cpp:707-722, 806-821. */
int shq_find_timesteps(shq_context *ctx, const shq_timestep_params *p, const int32_t *active, int64_t nactive, int64_t dti_min_global,
                       int mTimeBin_global, shq_timestep_result *res);
/* find_global_timestep (timestep.cpp:195-221): min over all live particles of the converted step; res->dti_min, res->nbadbin. */
int shq_find_global_timestep(shq_context *ctx, const shq_timestep_params *p, shq_timestep_result *res);
/* find_hydro_timesteps (timestep.cpp:583-703): TimeBinHydro of gas and BH on the list, capped by TimeBinGravity; BHs also get
 * TimeBinDynFric (get_timestep_dynfric_dloga, :1085-1110).  res->mintimebin carries the fix-ups of :677-696 for ONE rank; a
 * caller with several ranks reduces mTimeBin first and passes it back as mTimeBin_global to shq_set_bh_first_timestep. */
int shq_find_hydro_timesteps(shq_context *ctx, const shq_timestep_params *p, const int32_t *active, int64_t nactive, shq_timestep_result *res);
int shq_set_bh_first_timestep(shq_context *ctx, int mTimeBin);
/* hierarchical_gravity_and_timesteps, the three particle loops (timestep.cpp:356-380, 407-414, 449-464):
 * shq_hier_gravity_bins: TimeBinGravity = min(bin of the rounded-down gravity step, largest_active) and timebincounts;
 * shq_hier_push_down: TimeBinGravity = min(TimeBinGravity, push_down_bin) over the list;
 * shq_hier_refine: TimeBinGravity = ti - 1 where the step from the CURRENT level's acceleration is shorter than bin ti's
 *     (res->badstepsizecount counts them when ti == 1).
 * from_accel_store: the acceleration is the last walk's Accel output (AccelStore) instead of FullTreeGravAccel. */
int shq_hier_gravity_bins(shq_context *ctx, const shq_timestep_params *p, const int32_t *active, int64_t nactive, int from_accel_store,
                          int largest_active, shq_timestep_result *res);
int shq_hier_push_down(shq_context *ctx, const int32_t *active, int64_t nactive, int push_down_bin);
int shq_hier_refine(shq_context *ctx, const shq_timestep_params *p, const int32_t *active, int64_t nactive, int from_accel_store, int ti,
                    shq_timestep_result *res);
/* The sub-step levels of hierarchical_gravity_and_timesteps (timestep.cpp:417-476) in one call, resident: for ti = largest_active - 1
 * ... 1: sub-list (gravity bin <= ti) -> tree of the sub-list -> walk without potential -> shq_hier_refine -> hierarchical kick
 * Vel += Accel * gravkick_level[ti] (the caller's apply_hierarchical_grav_kick factor of level ti, :247-287, the lower level's kick
 * already subtracted).  Stops at the first empty sub-list (*mingravtimebin = ti + 1, :427-431; unchanged otherwise).
 * walk_mode: SHQ_WALK_EXACT / _GROUP / _AUTO for the level walks.  levels (may be NULL, capacity SHQ_TIMEBINS): what each level did. */
typedef struct shq_hier_level {
    int32_t timebin, walk_mode;       /* the level's bin; the walk it ran (what SHQ_WALK_AUTO resolved to) */
    int64_t nparticles, tree_nodes;   /* sub-list length = particles of the level's tree; its nodes */
    double tree_build_ms, walk_ms;    /* HIP-event times of the device tree build and of the walk kernel(s) */
} shq_hier_level;
int shq_hier_gravity_levels(shq_context *ctx, const shq_timestep_params *p, const shq_grav_params *gp, double BoxSize, int treemask,
                            int64_t Ti_Current, int largest_active, const double gravkick_level[SHQ_TIMEBINS + 1], int walk_mode,
                            int *mingravtimebin, int64_t *badstepsizecount, shq_hier_level *levels, int *nlevels);
/* get_long_range_timestep_dloga's particle loop (timestep.cpp:1153-1166): per type, sum of |Vel|^2, smallest positive mass and
 * count over the live particles.  The sum runs in a fixed order (blocks of 256 in index order, then the block sums in order),
 * so it is reproducible; the reference's OpenMP reduction has no fixed order. */
int shq_velocity_moments(shq_context *ctx, double v2sum[6], double min_mass[6], int64_t count[6]);
int shq_timebins_download(shq_context *ctx, uint8_t *bin_gravity, uint8_t *bin_hydro);
/* SphP[].MaxSignalVel by particle index (what the hydro criterion reads): upload for a state that did not come from a hydro
 * run of this context (NULL keeps it; gas particles only are read). */
int shq_maxsignalvel_upload(shq_context *ctx, const double *maxsignalvel_by_particle);
/* The gas state the SPH operators keep resident (Hsml, Vel, time bins, and per gas particle Entropy, DtEntropy, HydroAccel, DelayTime,
 * Density, EgyWtDensity, DhsmlEgyDensityFactor, DivVel, CurlVel, MaxSignalVel from its slot), without running one of them: what a
 * caller does before shq_fof (MaxDens / seed_index read Density and DelayTime) or shq_find_timesteps when no density / hydro call
 * preceded it in the step (e.g. right after a restart).  The particles must be the resident set. */
int shq_sph_state_upload(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph);

/* Particle exchange between tasks on opaque records (ExchangePlan, libgadget/exchange.hpp:31-537).
 * The arrays are the reference's own — particle_data[MaxPart] and the per-type slot arrays — through pointers the device can
 * read and write (shenqi allocates them managed; a port keeps them in HBM); records are copied as bytes, the library reads only
 * the flag byte, Type, PI and the slots' ReverseLink.  The collectives between the phases are the caller's.
 *   shq_exchange_plan   build_exchange_list (:158-176) + the counting half of build_export_buffer (:178-204): particles whose
 *                       d_target (layoutfunc, one int per particle) names another task, in index order, garbage / swallowed ones
 *                       excluded; the first min(nexchange, maxlast) of them (maxlast <= 0: all; find_iter_space is the caller's
 *                       memory policy) are counted into toGo[task] = {base, slots[6]}.
 *   shq_exchange_pack   the pack loop of exchange_once (:369-392): per target task the base records in list order into
 *                       d_partbuf at toGoOffset[task].base, the slot records of every enabled type in the same order into
 *                       d_slotbuf[type] at toGoOffset[task].slots[type]; then slots_mark_garbage on the source (IsGarbage,
 *                       ReverseLink = MaxPart + 100).
 *   shq_exchange_unpack after the caller's alltoallv put the arrivals behind NumPart / behind each slot array's size: PI of
 *                       every arrival renumbered in arrival order per source task and type (:483-511).
 * The slot compaction the reference may interleave (slots_gc when memory is short) stays with the caller. */
typedef struct shq_exchange_layout {
    size_t part_elsize, off_flags, off_type, off_pi;
    size_t slot_elsize[6];      /* 0: slot type not enabled */
    size_t off_reverselink;     /* particle_data_ext::ReverseLink, first member of every slot struct */
} shq_exchange_layout;
typedef struct shq_exchange_entry {   /* ExchangePlanEntry, exchange.hpp:18-21 */
    int64_t base;
    int64_t slots[6];
} shq_exchange_entry;
int shq_exchange_plan(shq_context *ctx, const shq_exchange_layout *layout, const void *d_parts, int64_t numpart, const int32_t *d_target,
                      int ThisTask, int NTask, int64_t maxlast, int64_t *nexchange, int64_t *last, shq_exchange_entry *toGo);
int shq_exchange_pack(shq_context *ctx, const shq_exchange_layout *layout, void *d_parts, void *const d_slots[6], int64_t MaxPart,
                      const shq_exchange_entry *toGoOffset, int NTask, void *d_partbuf, void *const d_slotbuf[6]);
int shq_exchange_unpack(shq_context *ctx, const shq_exchange_layout *layout, void *d_parts, int64_t numpart_old, const int64_t slot_size_old[6],
                        const shq_exchange_entry *toGet, const shq_exchange_entry *toGetOffset, int NTask);
/* slots_gc (libgadget/slotsmanager.cpp:132-370): garbage particles squeezed out of the particle array (order kept: slots_gc_base),
 * then for every slot type with compact[type] != 0: ReverseLink = particle index (invalid for garbage: slots_gc_mark), unreferenced
 * slots squeezed out in order (slots_gc_sweep), PI of the surviving particles renumbered (slots_gc_collect).  *numpart and
 * slot_size[] are updated.  What the exchange runs between pack and receive when memory is short (exchange.hpp:398-406).
 * Slot records of a type that is not compacted keep their places, as in the reference. */
int shq_slots_gc(shq_context *ctx, const shq_exchange_layout *layout, void *d_parts, int64_t *numpart, int64_t MaxPart, void *const d_slots[6],
                 int64_t slot_size[6], const int compact[6]);
/* slots_gc_sorted (libgadget/slotsmanager.cpp:417-510): the particle array sorted by type, then by Peano-Hilbert key, garbage
 * (TypeKey 255) last and trimmed off; every enabled slot array sorted by its particles' new positions (ReverseLink), unreferenced
 * slots trimmed, PI renumbered.  d_keys[i] = PEANO(Part[i].Pos, BoxSize) comes from the caller (shq_peano_keys, or its own key function: the
 * loop at :439-447); equal (type, key) pairs keep their order here (the reference's sort is unstable). */
int shq_slots_gc_sorted(shq_context *ctx, const shq_exchange_layout *layout, void *d_parts, int64_t *numpart, int64_t MaxPart, void *const d_slots[6],
                        int64_t slot_size[6], const uint64_t *d_keys);

/* slots_split_particle and slots_convert (libgadget/slotsmanager.cpp:27-126) for lists of particles: what star formation does
 * with NewStars / NewParents (sfr_eff.cpp:344-372, placement = firststarslot + i), black-hole seeding (blackhole.cpp:1040) and the
 * wind spawns do one particle at a time.  The reference hands out new particle and slot indices with atomic counters, so their
 * order is the threads'; here entry k of the list gets NumPart + k / slot_size + k.  All pointers except the size arrays are device
 * pointers; the entries of a list must be distinct.
 *   shq_slots_split_particles   entry k: Generation of the parent ++ (4 bits of the flag byte, wrapping as the bit field does),
 *                               Base[NumPart + k] = Base[parent], child ID = (ID & 0x00ff..ff) + (Generation << 56), child Mass =
 *                               childmass[k], parent Mass -= childmass[k] (float, formed in double), child PI = -1; *numpart += n;
 *                               d_children (may be NULL) receives the new indices.  SHQ_ERR_NOMEM when NumPart + n > MaxPart
 *                               ("Tried to spawn ... no space left", :107), nothing touched.
 *   shq_slots_convert           entry k: the old slot (if the old type has slots and PI >= 0) gets ReverseLink = MaxPart + 100, a new
 *                               slot of ptype at slot_size[ptype] + k is filled with the poison byte 101 (slots_connect_new_slot)
 *                               and becomes the particle's PI, Type = ptype; slot_size[ptype] += n.  A ptype without slots only
 *                               changes Type.  SHQ_ERR_NOMEM when the new slots would pass slot_maxsize[ptype] ("Tried to use
 *                               non-allocated slot", :76): reserving is the caller's (sfr_reserve_slots, fof_seed), before the call. */
typedef struct shq_spawn_layout {
    size_t off_id, off_mass;    /* particle_data::ID (uint64), ::Mass (float) */
    int generation_shift;       /* first bit of the 4-bit Generation field inside the flag byte at shq_exchange_layout::off_flags */
    int pad_;
} shq_spawn_layout;
int shq_slots_split_particles(shq_context *ctx, const shq_exchange_layout *layout, const shq_spawn_layout *spawn, void *d_parts, int64_t *numpart,
                              int64_t MaxPart, const int32_t *d_parents, const double *d_childmass, int64_t n, int32_t *d_children);
int shq_slots_convert(shq_context *ctx, const shq_exchange_layout *layout, void *d_parts, int64_t numpart, int64_t MaxPart, void *const d_slots[6],
                      int64_t slot_size[6], const int64_t slot_maxsize[6], const int32_t *d_index, int64_t n, int ptype);

/* Scope note: this entry is the slot-manager side of star formation — the one place where slots_convert / slots_split_particle
 * (the row these belong to) have to fill a freshly converted slot from another slot array while both stay in HBM.
 * Nothing here evaluates star-formation physics: who forms a star is decided by the caller, or per particle by the engine of the
 * "star formation" block at the end of this header (shq_sfr_eval: the sfr_eff.cpp criteria, the eeqos relaxation, the random draws).
 * make_particle_star (libgadget/sfr_eff.cpp:604-630) for the lists of the star-formation merge step (:344-372): entry k converts
 * children[k] (the parent itself, or the particle split off it) to a star at slot firststarslot + k and fills the slot from the
 * PARENT's gas slot as it was before the conversion: FormationTime = Time, LastEnrichmentMyr = TotalMassReturned = 0, BirthDensity,
 * VDisp, Metallicity, Metals[nmetals].  A parent that is not gas is SHQ_ERR_INVALID ("Only gas forms stars"), nothing touched.
 * Field types are the reference's (star: float FormationTime / LastEnrichmentMyr / BirthDensity / VDisp / Metals, double
 * TotalMassReturned / Metallicity; gas: double Density / VDisp / Metallicity, float Metals). */
typedef struct shq_star_spawn_layout {
    size_t star_formationtime, star_lastenrichmentmyr, star_totalmassreturned, star_birthdensity, star_vdisp, star_metallicity, star_metals;
    size_t sph_density, sph_vdisp, sph_metallicity, sph_metals;
    int nmetals, pad_;
} shq_star_spawn_layout;
int shq_make_particle_stars(shq_context *ctx, const shq_exchange_layout *layout, const shq_star_spawn_layout *sl, void *d_parts, int64_t numpart, int64_t MaxPart,
                            void *const d_slots[6], int64_t slot_size[6], const int64_t slot_maxsize[6], const int32_t *d_children, const int32_t *d_parents,
                            int64_t n, double Time);
/* blackhole_make_one (libgadget/blackhole.cpp:1029-1088) for a list of gas particles (fof_seed's ImportGroups[n].seed_index,
 * fof.cpp:1378-1381): conversion to type 5 + every field the reference initialises; seedmass[k] is BHP.Mass = Mseed
 * (SeedBlackHoleMass, or the caller's bh_powerlaw_seed_mass(ID) draw); with SeedBHDynMass > 0 the particle's mass moves to Mtrack
 * and becomes SeedBHDynMass, otherwise Mtrack = -1.  Not gas: SHQ_ERR_INVALID ("Only Gas turns into blackholes"). */
typedef struct shq_bh_seed_layout {
    size_t bh_mass, bh_mseed, bh_mdot, bh_formationtime, bh_swallowid, bh_density, bh_timebindynfric, bh_minpotpos, bh_dfaccel, bh_df_surroundingvel,
        bh_dragaccel, bh_df_surroundingrmsvel, bh_df_surroundingdensity, bh_jumptominpot, bh_countprogs, bh_mtrack, bh_kineticfdbkenergy, bh_vdisp;
    size_t part_pos, part_mass, part_timebin_hydro;
} shq_bh_seed_layout;
int shq_blackhole_make_seeds(shq_context *ctx, const shq_exchange_layout *layout, const shq_bh_seed_layout *bl, void *d_parts, int64_t numpart, int64_t MaxPart,
                             void *const d_slots[6], int64_t slot_size[6], const int64_t slot_maxsize[6], const int32_t *d_index, const double *d_seedmass, int64_t n,
                             double atime, double SeedBHDynMass);

/* Friends-of-friends groups of the resident particles (the first legacy-API user: libgadget/fof.cpp, one task).
 *   fof_label_primary (:368-581): particles of the primary types within LinkingLength of each other (r2 <= L^2, the neighbour
 *       test of treewalk_visit_ngbiter, treewalk.c:946-961) are one group; the reference's lock-free union-find (fofp_merge,
 *       update_root) ends in the connected components labelled with their smallest particle ID, and so does this one
 *       (atomicCAS hooking of the larger root under the smaller, path halving, one pass over a tree of the primary types);
 *   fof_label_secondary (:1142-1270): every particle of the secondary types takes the label of the nearest primary particle within
 *       a search radius that starts at max(0.4 L, 0.5 Hsml) (float) and doubles while it is below 4 L; ties go to the particle met
 *       first in the tree's depth-first order, as in the reference's nolist walk;
 *   fof_fof / fof_compile_base / fof_assign_grnr / add_particle_to_group / fof_finish_group_properties (:159-256, 583-766, 1048-1096):
 *       particles sorted by label, groups shorter than HaloMinLength dropped, GrNr = 1.. by decreasing length then MinID,
 *       Length / LenType / MassType / Mass / CM / Vel / Imom / Jmom / MaxDens + seed_index per group, groups ordered by MinID.
 * The reference's sort of the labels is not stable, so which member is FirstPos and the order of a group's sums are unspecified
 * there; here the member with the lowest particle index comes first and sums run in index order (one thread per group: deterministic).
 * The slot-resident sums (Sfr, metal masses, BH_Mass / BH_Mdot) stay with the caller: shq_fof_members hands it every group's member
 * list.  Several tasks (ghost labels through the export walk, fof_reduce_groups) are not covered.
 * shq_fof builds its own tree over the primary types (force_tree_rebuild_mask(&dmtree, ..., FOFPrimaryLinkTypes)) in the context's
 * tree storage and leaves the context WITHOUT a resident tree, as fof_fof frees its tree (fof.cpp:254): the next gravity / SPH /
 * export call needs shq_tree_build or shq_tree_upload first and returns SHQ_ERR_STATE otherwise.
 * ids: Part[].ID by particle index (host).  minid_by_particle / grnr_by_particle (host, may be NULL): HaloLabel[].MinID and Part[].GrNr
 * (-1 outside groups).  WindsDecoupleSph: winds_is_particle_decoupled applies (DelayTime > 0 gas never seeds). */
typedef struct shq_fof_params {
    double BoxSize;
    double LinkingLength;       /* FOFHaloComovingLinkingLength */
    int32_t PrimaryLinkTypes, SecondaryLinkTypes;   /* type masks */
    int32_t HaloMinLength;
    int32_t WindsDecoupleSph;
} shq_fof_params;
typedef struct shq_fof_group {
    uint64_t MinID;
    int32_t Length, GrNr;
    int32_t LenType[6];
    float FirstPos[3];
    int32_t seed_index;
    double MassType[6];
    double Mass;
    double CM[3];
    double Vel[3];
    double Imom[3][3];
    double Jmom[3];
    double MaxDens;
    int64_t first_member;       /* offset of the group's members in the list of shq_fof_members */
} shq_fof_group;
int shq_fof(shq_context *ctx, const shq_fof_params *params, const uint64_t *ids, uint64_t *minid_by_particle, int32_t *grnr_by_particle,
            int64_t *ngroups);
int shq_fof_groups_download(shq_context *ctx, shq_fof_group *groups, int64_t capacity);
/* The slot-resident sums of add_particle_to_group (fof.cpp:599-618: MassHeIonized, Sfr, GasMetalMass, GasMetalElemMass[],
 * StellarMetalMass, StellarMetalElemMass[], BH_Mdot, BH_Mass): per group and column the sum of values_by_particle[i][col] over the
 * group's members, in member (particle index) order.  The caller fills the columns from its slots (zero where a type does not
 * contribute); sums_by_group is [ngroups][ncol] in catalogue order.  Groups of more than 256 members are summed in 256 slices. */
int shq_fof_group_sums(shq_context *ctx, const double *values_by_particle, int ncol, double *sums_by_group);
/* The marking loop of fof_seed (fof.cpp:1290-1302) on the resident catalogue: the seed_index (densest gas particle) of every group
 * with Mass >= MinFoFMassForNewSeed, MassType[4] >= MinMStarForNewSeed, no black hole yet and a seed candidate, in catalogue order,
 * into the DEVICE array d_seed_index (NULL: count only) — the list shq_blackhole_make_seeds takes.  One task: seed_task is this task. */
int shq_fof_seed_select(shq_context *ctx, double MinFoFMassForNewSeed, double MinMStarForNewSeed, int32_t *d_seed_index, int64_t capacity, int64_t *nseeds);
/* particle indices of all kept groups, group after group (order of shq_fof_groups_download), members in index order */
int shq_fof_members(shq_context *ctx, int32_t *members, int64_t capacity, int64_t *nmembers);

/* Black-hole slot fields of the resident step (bh_particle_data, slotsmanager.h:35-73).  With them on the device
 * shq_drift repositions a BH with JumpToMinPot set (drift.cpp:32-53, when shq_set_bh_reposition is on), shq_kick_hydro adds
 * the dynamic-friction and drag kicks (timestep.cpp:973-979, factor bh_gravkick[TimeBinHydro] as apply_half_kick passes it),
 * the time-step loops read minTimeBin and write TimeBinDynFric.  download writes TimeBinDynFric and JumpToMinPot back. */
typedef struct shq_bh_dyn_view {
    void *base;
    size_t elsize;
    int64_t numslots;
    size_t off_mintimebin, off_timebindynfric, off_jumptominpot;       /* unsigned char, unsigned char, char */
    size_t off_dfaccel, off_df_surroundingvel, off_dragaccel;         /* MyFloat[3] (double) */
    size_t off_minpotpos, off_minpotvel;                              /* double[3], MyFloat[3] */
} shq_bh_dyn_view;
int shq_bh_dynamics_upload(shq_context *ctx, const shq_part_view *parts, const shq_bh_dyn_view *bh);
int shq_bh_dynamics_download(shq_context *ctx, const shq_part_view *parts, const shq_bh_dyn_view *bh);
int shq_set_bh_reposition(shq_context *ctx, int enabled);
int shq_kick_bh(shq_context *ctx, const double gravkick[SHQ_TIMEBINS + 1], const int32_t *active, int64_t nactive);
/* active: host int32 list or NULL. The walk and postprocess are queued on the stream. */
int shq_grav_short_run(shq_context *ctx, const shq_grav_params *params, const int32_t *active,
                       int64_t nactive, int update_potential, int walk_mode);
/* The same walk + postprocess for the own particles [first, first + count) without a list: a piece of the work-set
 * TreeWalk::run_on_queue (libgadget/treewalk2.h:282-330) is given.  The pieces of one evaluation must start at first = 0 and
 * together cover what shq_grav_short_run(active = NULL) covers; their interaction statistics add up (kernel_ms is the last
 * piece's).  Lets the caller queue other work on the stream between the pieces. */
int shq_grav_short_run_range(shq_context *ctx, const shq_grav_params *params, int64_t first, int64_t count,
                             int update_potential, int walk_mode);
/* Copy results back: accel[numpart][3] (may be NULL), potential[numpart] (may be NULL),
 * ninteractions[numpart] (may be NULL). Synchronises. */
/* Wave-level walk counters in shq_walk_stats (nnodes_visited, nwave_*, nnode_interactions): 0 off (default: they stay
 * zero; the counters cost the walk ~4 %, they press on its scalar register budget), 1 on, 2 plus per-lane-participation
 * histograms printed to stderr.  ninteractions, min / max and kernel_ms are always filled. */
int shq_set_walk_stats(shq_context *ctx, int level);
/* How shq_grav_short_run launches the exact primary walk (a tuning / test knob; results are the same interaction sets either way).
 * persist: 0 one 64-target task per wave; 1 (default) persistent waves taking tasks from per-XCD counters once the launch exceeds
 * what the chip holds at once; 2 persistent waves for every launch.  leaf_ring: 1 (default) leaf particles go through the
 * wave-private LDS ring of the persistent walk, 0 they are evaluated as the leaf is opened (the reference's summation order). */
int shq_set_walk_launch(shq_context *ctx, int persist, int leaf_ring);
/* The production launch (persistent waves + leaf ring, relative criterion) does not enter a subtree that at most twelve (SHQ_SPARSE_LANES; eight before DESIGN 3.1 round 7) of a wave's 64
 * lanes open: it notes it, and a second kernel walks the noted subtrees with one lane per (target, node) pair: the
 * same interaction sets, a different order of the sum (forces to 1e-13 of the largest).  On by default; 0 (or SHQ_WALK_SPARSE=0)
 * makes the main walk enter every subtree itself.  A test / tuning knob like shq_set_walk_launch.
 * The pair kernel fetches the first 80 bytes of a node's record and recomputes the products of {mass, len} and the walk parameters that
 * fill the rest (same expressions, same bits) whenever the device found that true of every record of the pool when it last filled
 * them; 2 makes it fetch whole records regardless.  shq_walk_pair_lean: 1 if the current pool passed that check, 0 if not (or not
 * checked yet), < 0 on error. */
int shq_set_walk_sparse(shq_context *ctx, int enable);
int shq_walk_pair_lean(shq_context *ctx);
/* Where the pair kernel runs: 1 (default; SHQ_WALK_OVERLAP) beside the main walk on the context's second stream once a launch has
 * at least 128 tasks per CU — three workgroups of the main walk and one of the pair kernel per CU, the pair kernel taking a task when
 * the main walk has raised its flag (results, noted subtrees and OldAcc cross at the device's coherence point); 0 behind it on the
 * same stream; 2 beside it whatever the size of the launch (tests).  Same interaction sets and the same sums in every mode. */
int shq_set_walk_overlap(shq_context *ctx, int mode);
/* How the production launch (persistent waves + leaf ring + sparse hand-over, relative criterion, no fused readout) addresses the node
 * pool: 1 (default; SHQ_WALK_ADDR) a record's byte offset in one 32-bit register wherever the pool allows it, 0 always the 64-bit
 * address.  Every other launch form uses the 64-bit address.  The same loads of the same records: results are equal bit for bit.  A
 * test / tuning knob like shq_set_walk_launch.
 * shq_walk_addr32_fits: the rule, on numbers alone: 1 if a pool of numnodes + 1 records of 128 bytes lies within reach of the 32-bit
 * offset (numnodes + 1 <= 2^25), else 0.  shq_walk_last_addr: 1 if the last exact walk launched fetched its records by 32-bit offset. */
int shq_set_walk_addr(shq_context *ctx, int mode);
int shq_walk_last_addr(shq_context *ctx, int *mode);
int shq_walk_addr32_fits(int64_t numnodes);
/* The pair kernel has a 32-bit form of its own (scalar base + 32-bit lane offset for node records, the leaf-ordered particle copy and the
 * wave's pair stack), taken under the same knob where all three fit.  shq_pair_addr32_fits: the rule on numbers alone: 1 if
 * shq_walk_addr32_fits(numnodes), leaf_slots slots of 32 bytes and stack_cap stack entries of 16 bytes all end at or below 2^32.
 * shq_walk_last_pair_addr: 1 if the last pair kernel launched took that form.  Same pairs, same order: results equal bit for bit. */
int shq_pair_addr32_fits(int64_t numnodes, int64_t leaf_slots, int64_t stack_cap);
int shq_walk_last_pair_addr(shq_context *ctx, int *mode);
/* The pair kernel's failures are STICKY and loud (the reference checks every launch and ends the run, treewalk2.cuh:351-353).
 *  - A pair stack that ran full dropped pairs: the accelerations of that launch are incomplete.  The error word stays up on the device
 *    whatever is launched afterwards; a copy follows every launch to pinned host memory, and shq_synchronize, every *_download,
 *    shq_kick_short, shq_hier_refine, shq_walk_pair_status (which wait for the stream) and the next shq_treepm_step /
 *    shq_grav_short_run (which do not: they see the launches completed by then) return SHQ_ERR_DEVICE once; the report clears it.
 *  - A wave of the pair kernel running BESIDE the main walk that gave up waiting for a task (the two kernels were not co-resident:
 *    nothing in HIP promises they are) is not an error any more: a mop-up pass behind both kernels walks every task not marked done,
 *    in the order of the pair kernel run behind the walk (same sums, same bits).  It returns at once when nobody gave up.
 * shq_walk_pair_status: launches since shq_init that needed the mop-up pass, the deepest pair stack seen (entries, of SHQ_SPARSE_STACK
 * = 4096 per wave), the tasks the last launch's mop-up walked; waits for the stream and returns the sticky error like the others.
 * shq_set_walk_debug (tests): pair_spin_max > 0 = polls of a task's flag before a live pair wave gives up (default 2^22; 1 starves
 * it: every task goes to the mop-up pass); pair_stack_cap > 0 = pairs per wave stack (1344 .. 4096; small values force the overflow). */
int shq_walk_pair_status(shq_context *ctx, int64_t *recovered_launches, int64_t *stack_high_water, int64_t *last_mopped_tasks);
int shq_set_walk_debug(shq_context *ctx, int pair_spin_max, int pair_stack_cap);
/* shq_set_tree_debug (tests): initial_node_cap > 0 = node pool of the first attempt of every later shq_tree_build /
 * shq_tree_build_domain (0: the default 0.6 n + 4096).  A tree that does not fit ends the attempt on the device (nothing is written
 * past the pool or the frontier, no later level runs); the host doubles the pool and builds again, up to 5 attempts, then returns
 * SHQ_ERR_NOMEM ("node pool overflow") with no tree installed.  Small values force that retry path; the tree is the same.
 * shq_tree_build_attempts: attempts the last build made (1 = no retry). */
int shq_set_tree_debug(shq_context *ctx, int64_t initial_node_cap);
int shq_tree_build_attempts(shq_context *ctx, int *attempts);
/* Checker utility: direct summation as the reference's own gravity test does it (force_direct / grav_force,
 * libgadget/tests/test_gravity.cpp:41-76,121-143): accel[ns][3] (host) = acceleration at the ns sample positions (host, [ns][3]) from
 * the first nsrc resident particles and their (2 repeat + 1)^3 periodic images, spline-softened below h.  Partial sums over a
 * rank's local particles add up across ranks (bench.py's sampled force check of the sharded TreePM step). */
int shq_direct_force_sample(shq_context *ctx, const double *sample_pos, int64_t ns, int64_t nsrc, double BoxSize, double G, double h,
                            int repeat, double *accel);
int shq_grav_short_download(shq_context *ctx, double (*accel)[3], double *potential,
                            int64_t *ninteractions, shq_walk_stats *stats);
/* Secondary walk: TreeWalk::ev_secondary (libgadget/treewalk2.h:618-700) with GravLocalTreeWalk::visit
 * <TREEWALK_GHOSTS> (gravshort2.hpp:243-322).  `queries` are the imported GravTreeQuery records of other ranks'
 * particles (binary mirror: Pos[3], NodeList[NODELISTLENGTH = 4], OldAcc; gravshort2.hpp:123-128,
 * localtreewalk2.h:76-115); each walks the branches under the top-level nodes of its NodeList (node numbers
 * of the uploaded tree, -1 terminated) of the context's current tree and particles.  `results` receive the raw
 * GravTreeResult sums (Acc not multiplied by G, Potential without the self term: the exporting rank reduces and
 * post-processes them, treewalk2.h:780-812).  Synchronous; host pointers.  With this entry point the library
 * also serves under shenqi's own export / import machinery on multi-rank runs. */
typedef struct shq_grav_query {
    double Pos[3];
    int32_t NodeList[4];
    double OldAcc;
} shq_grav_query;
typedef struct shq_grav_result {
    double Acc[3];
    double Potential;
} shq_grav_result;
int shq_grav_short_secondary(shq_context *ctx, const shq_grav_params *params, const shq_grav_query *queries, int64_t nq,
                             shq_grav_result *results, int64_t *ninteractions, int update_potential);
/* ---- top-tree walk: which remote top-leaves must a target visit ----
 * The reference's ev_count_exports + ev_toptree (treewalk2.cuh:243-334) for the host's own export / import
 * machinery (treewalk2.h:618-812): per target, walk only the TopLevel nodes of the host tree; every pseudo node
 * that the walk would open becomes an export, consecutive leaves of one task coalescing into NodeList[4]
 * (TopTreeWalk::export_particle / export_count, localtreewalk2.h:269-324).
 *
 * shq_toptree_upload: the TopLevel nodes of `tree` and the domain's TopLeaves table (pseudo node suns[0] - lastnode
 *     indexes it).  Only needed when the tree has pseudo nodes; independent of shq_tree_upload.
 * shq_grav_toptree_exports: GravTopTreeWalk::toptree_visit (gravshort2.hpp:362-438) for the resident targets
 *     (positions, OldAcc as for shq_grav_short_run).
 * shq_ngb_toptree_exports: TopTreeWalk::toptree_visit with cull_node<symmetric> (localtreewalk2.h:154-182, 210-259),
 *     search radius = the resident Hsml (density: symmetric 0; hydro: symmetric 1, needs the top nodes' hmax).
 * Outputs: exportcounts[t] = inclusive running total of exports up to target t (the reference's scanned
 * exportcounts, used by its BunchSize logic; may be NULL); table = the DataIndexTable, target t's entries contiguous at
 * [exportcounts[t-1], exportcounts[t]) in the reference's order; *nexport always returns the total.  With table == NULL
 * only counts are produced; with capacity < total nothing is written and SHQ_ERR_NOMEM is returned. */
typedef struct shq_data_index { /* struct data_index, libgadget/localtreewalk2.h:188-193 */
    int32_t Task;
    int32_t Index;
    int32_t NodeList[4];
} shq_data_index;
int shq_toptree_upload(shq_context *ctx, const shq_tree_view *tree, const shq_topleaf *topleaves, int ntopleaves);
int shq_grav_toptree_exports(shq_context *ctx, const shq_grav_params *params, const int32_t *active, int64_t nactive,
                             int32_t *exportcounts, shq_data_index *table, int64_t capacity, int64_t *nexport);
int shq_ngb_toptree_exports(shq_context *ctx, int symmetric, double BoxSize, const int32_t *active, int64_t nactive,
                            int32_t *exportcounts, shq_data_index *table, int64_t capacity, int64_t *nexport);
/* The same export detection with everything left in HBM (what ev_count_exports + ev_toptree do on managed memory,
 * treewalk2.cuh:243-334): active = NULL (all own particles), a resident handle, or — active_on_device != 0 — a DEVICE list.  Back
 * come the number of exports and task_counts[ntask], the entries per destination task (the send counts of
 * ev_send_recv_export_import, treewalk2.h:618-700); the table stays resident.  shq_grav_export_pack then writes, on the device,
 * the GravTreeQuery records of the table in task order (entries of one task in table order) into d_queries and the particle
 * index of every record into d_place (the `place` argument of shq_grav_reduce_export_results): the send buffer of the caller's
 * all-to-all, never on the host. */
int shq_grav_toptree_exports_resident(shq_context *ctx, const shq_grav_params *params, const int32_t *active, int64_t nactive,
                                      int active_on_device, int ntask, int64_t *nexport, int64_t *task_counts);
int shq_grav_export_pack(shq_context *ctx, shq_grav_query *d_queries, int32_t *d_place);
/* GravTreeResult::reduce<TREEWALK_GHOSTS> (gravshort2.hpp:136-146) for n returned results: Accel[place[k]] += results[k].Acc
 * and, with update_potential, Potential likewise, in the order k = 0..n-1 (the reference's loop over its export table, so
 * a target's partial sums are added in the same order).  Needs a preceding shq_grav_short_run with
 * SHQ_WALK_DEFER_POSTPROCESS.  shq_grav_postprocess: GravTreeOutput::postprocess (gravshort2.hpp:88-107) for the
 * targets of that run (same active argument). */
int shq_grav_reduce_export_results(shq_context *ctx, const int32_t *place, const shq_grav_result *results, int64_t n,
                                   int update_potential);
int shq_grav_postprocess(shq_context *ctx, const shq_grav_params *params, const int32_t *active, int64_t nactive,
                         int update_potential);
/* Set the per-particle OldAcc inputs on the device from the device-resident
 * FullTreeGravAccel + GravPM of the last shq_grav_short_run / shq_pm_run
 * (grav_get_abs_accel, gravshort2.hpp:111-121). */
int shq_grav_refresh_oldacc(shq_context *ctx, double G);

/* ---- SPH density and hydro force ------------------------------------------------------- */

#define SHQ_DENSITY_KERNEL_CUBIC_SPLINE 1   /* enum DensityKernelType, libgadget/density2.h */
#define SHQ_DENSITY_KERNEL_QUINTIC_SPLINE 2
#define SHQ_DENSITY_KERNEL_QUARTIC_SPLINE 4

/* POD mirror of KickFactorData (libgadget/density2.h:52-129): the host (timebinmgr) fills it. */
typedef struct shq_kick_factors {
    double FgravkickB;
    double gravkicks[SHQ_TIMEBINS + 1];
    double hydrokicks[SHQ_TIMEBINS + 1];
    double dloga_kick[SHQ_TIMEBINS + 1];
    double dloga_for_bin[SHQ_TIMEBINS + 1];
} shq_kick_factors;

/* POD mirror of DensityPriv + the density_params it reads (libgadget/densitytree2.hpp:10-52,
 * density2.h:16-33). */
typedef struct shq_density_params {
    double BoxSize;
    double DesNumNgb;           /* GetNumNgb(kernel) */
    double DesNumNgbBH;         /* DesNumNgb * BlackHoleNgbFactor */
    double MinGasHsml;
    double MaxNumNgbDeviation;
    int32_t update_hsml;
    int32_t BlackHoleOn;
    int32_t DoEgyDensity;
    int32_t WindsDecouple;      /* winds_ever_decouple() */
    int32_t DensityKernelType;
    int32_t pad_;
    shq_kick_factors kf;
} shq_density_params;

/* POD mirror of HydroPriv (libgadget/hydratree2.hpp:60-125). */
typedef struct shq_hydro_params {
    double BoxSize;
    double atime;
    double fac_mu;              /* pow(atime, 3(GAMMA-1)/2) / atime */
    double fac_vsic_fix;        /* hubble * pow(atime, 3 GAMMA_MINUS1) */
    double hubble_a2;           /* hubble * atime^2 */
    double drifts[SHQ_TIMEBINS + 1];
    double ArtBulkViscConst;
    double DensityContrastLimit;
    double WindSpeed;
    double WindFreeTravelDensThresh;
    int32_t DensityIndependentSphOn;
    int32_t DensityKernelType;
    shq_kick_factors kf;
} shq_hydro_params;

/* View of the BH slots density() writes for Type-5 targets (bh_particle_data.Density/.DivVel). */
typedef struct shq_bh_view {
    void *base;
    size_t elsize;
    int64_t numslots;
    size_t off_density, off_divvel;
} shq_bh_view;

typedef struct shq_sph_stats {
    int64_t ntargets;
    int64_t ninteractions;   /* ngbiter calls summed over targets and iterations */
    int32_t niterations;     /* Hsml iterations (do_hsml_loop, treewalk2.h:480-557) */
    int32_t pad_;
    double kernel_ms;        /* HIP-event time of the walk kernels */
    double hsml_max_tried;   /* density and stellar-density calls: the largest Hsml any walk of the loop searched with or any target ends
                                with (a collapsed bracket ends on Right, a floor on MinGasHsml: radii no walk ran with; stellar density: the
                                largest of its trial radii); 0 for other operators.  A sharded
                                caller sizes its ghost halo by this, not by the Hsml the loop ends with: an intermediate guess beyond the
                                halo undercounts NumNgb and steers the iteration (treewalk2.h:480-557 runs every guess against all ranks) */
} shq_sph_stats;

/* One-shot replacement of density_cuda() *including* the host Hsml loop the reference keeps on
 * the CPU (do_hsml_loop + DensityOutput::postprocess + density_check_neighbours,
 * treewalk2.h:480-557, densitytree2.hpp:117-257).  Targets: active particles of Type 0 / 5 that
 * are neither garbage nor swallowed (DensityQuery::haswork).  Writes Part[].Hsml / DtHsml,
 * SphP[].Density / EgyWtDensity / DhsmlEgyDensityFactor / DivVel / CurlVel, BhP[].Density /
 * DivVel, and - as update_tree_hmax_father does (forcetree.cpp:1285-1313) - raises mom.hmax of
 * the leaf holding each finished target in the caller's NODE array.  EntVarPred[numslots]
 * (out, may be NULL) receives the predicted entropy variable handed to hydro
 * (density2.cpp:147); GradRho_mag[numslots] (out, may be NULL) |grad rho| (density2.cpp:135-143).
 * Returns SHQ_ERR_NOCONV if MAXITER (400) is exceeded. */
int shq_density(shq_context *ctx, const shq_tree_view *tree, shq_node *nodes_rw,
                const shq_part_view *parts, const shq_sph_view *sph, const shq_bh_view *bh,
                const int32_t *active, int64_t nactive, const shq_density_params *params,
                double *EntVarPred, double *GradRho_mag, shq_sph_stats *stats);

/* One-shot replacement of hydro_force_cuda(): symmetric neighbour walk (cull radius
 * max(hmax_node, Hsml_i)), HydroResult::reduce and HydroOutput::postprocess
 * (hydratree2.hpp:127-149,201-379).  Writes SphP[].HydroAccel / DtEntropy / MaxSignalVel for
 * the active Type-0 targets.  EntVarPred may be NULL (then computed per particle).
 * A target's time bin must have params->drifts[bin] == 0, as the HydroPriv ctor leaves it for active bins
 * (hydratree2.hpp:94-100): the query takes the target un-drifted; otherwise SHQ_ERR_INVALID (shq_hydro_open too). */
int shq_hydro_force(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts,
                    const shq_sph_view *sph, const int32_t *active, int64_t nactive,
                    const shq_hydro_params *params, const double *EntVarPred, shq_sph_stats *stats);

/* ---- SPH walks in phases: the reference's distributed walk (treewalk2.h:277-373, do_hsml_loop :480-557) ----------
 * shq_density / shq_hydro_force above are  open -> { ev_primary -> ev_postprocess } -> close  in one call.  A multi-rank
 * run under shenqi's own export / import machinery drives the same phases itself — they are the hooks a TreeWalk
 * backend overrides (treewalk2.cuh:212-394) — and inserts the exchange between ev_primary and ev_postprocess:
 *
 *   shq_density_open(...)                        upload, predicted velocities, Left/Right bounds, work queue (haswork)
 *   repeat:
 *     shq_density_ev_primary(ctx)                raw sums of the queue's targets over the local tree (pseudo nodes skipped)
 *     shq_sph_exports(ctx, ...)                  top-tree walk of the queue with its current Hsml -> data_index table
 *                                                (needs shq_toptree_upload; symmetric for hydro)
 *     shq_sph_fill_queries(ctx, table, n, q)     DensityQuery / HydroQuery records of the table's entries
 *     ... MPI: queries out, other ranks' queries in ...
 *     shq_density_ev_secondary(ctx, ...)         visit<TREEWALK_GHOSTS> of imported queries against the local tree: raw
 *                                                DensityResult sums (any rank may call this while its own walk is open)
 *     ... MPI: results back ...
 *     shq_density_ev_reduce(ctx, place, res, n)  DensityResult::reduce<TREEWALK_GHOSTS>, entries of a target in order
 *     shq_density_ev_postprocess(ctx, &nredo)    DensityOutput::postprocess + Hsml update; nredo = targets to redo
 *   until every rank reports nredo == 0 (ranks with an empty queue keep serving secondaries)
 *   shq_density_close(...)                       results back into the caller's arrays
 *
 * Hydro is the same with one pass.  The structs are binary mirrors of DensityQuery / DensityResult
 * (densitytree2.hpp:260-344) and HydroQuery / HydroResult (hydratree2.hpp:151-228). */
typedef struct shq_density_query {
    double Pos[3];
    int32_t NodeList[4];
    double Vel[3];
    double Hsml;
    int32_t Type;
    int32_t pad_;
} shq_density_query;               /* 80 bytes */
typedef struct shq_density_result {
    double EgyRho, DhsmlEgyDensity, Rho, DhsmlDensity, Ngb, Div;
    double Rot[3];
    double GradRho[3];
} shq_density_result;              /* 96 bytes */
typedef struct shq_hydro_query {
    double Pos[3];
    int32_t NodeList[4];
    double EgyRho, EntVarPred;
    double Vel[3];
    double Hsml, Mass, Density, Pressure, F1, SPH_DhsmlDensityFactor;
    int32_t TimeBinHydro;
    int32_t pad_;
} shq_hydro_query;                 /* 136 bytes */
typedef struct shq_hydro_result {
    double Acc[3];
    double DtEntropy, MaxSignalVel;
} shq_hydro_result;                /* 40 bytes */

int shq_density_open(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph,
                     const shq_bh_view *bh, const int32_t *active, int64_t nactive, const shq_density_params *params,
                     int want_gradrho, int64_t *nqueue);
int shq_density_ev_primary(shq_context *ctx);
int shq_density_ev_secondary(shq_context *ctx, const shq_density_params *params, const shq_density_query *queries, int64_t nq,
                             shq_density_result *results, int64_t *ninteractions_total);
int shq_density_ev_reduce(shq_context *ctx, const int32_t *place, const shq_density_result *results, int64_t n);
int shq_density_ev_postprocess(shq_context *ctx, int64_t *nredo);
int shq_density_close(shq_context *ctx, shq_node *nodes_rw, const shq_part_view *parts, const shq_sph_view *sph,
                      const shq_bh_view *bh, double *EntVarPred, double *GradRho_mag, shq_sph_stats *stats);

int shq_hydro_open(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph,
                   const int32_t *active, int64_t nactive, const shq_hydro_params *params, const double *EntVarPred,
                   int64_t *nqueue);
int shq_hydro_ev_primary(shq_context *ctx);
int shq_hydro_ev_secondary(shq_context *ctx, const shq_hydro_params *params, const shq_hydro_query *queries, int64_t nq,
                           shq_hydro_result *results, int64_t *ninteractions_total);
int shq_hydro_ev_reduce(shq_context *ctx, const int32_t *place, const shq_hydro_result *results, int64_t n);
int shq_hydro_ev_postprocess(shq_context *ctx);
int shq_hydro_close(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, shq_sph_stats *stats);

/* ---- the SPH operators on a gas set that is already in HBM (sharded runs: local + imported ghost gas as rows of a device buffer
 * that came out of the all-to-all; shenqi_amd/dist.py DistSPHDevice) -----------------------------------------------------------
 * A row holds what density() / hydro_force() read of a neighbour and write of a target, SHQ_GAS_NCOL doubles:
 *    0-2 Pos   3 Mass   4-6 Vel   7 Hsml   8-10 FullTreeGravAccel   11-13 GravPM   14-16 HydroAccel   17 Entropy   18 DtEntropy
 *    19 DelayTime   20 Density   21 EgyWtDensity   22 DhsmlEgyDensityFactor   23 DivVel   24 CurlVel   25 MaxSignalVel   26 DtHsml
 *    27 TimeBinGravity + 256 TimeBinHydro (as a double)
 * shq_gas_set_device : the n rows become the resident particle set (all Type 0; the first nlocal are this rank's own = the
 *                      targets); any tree is dropped: shq_tree_build(ctx, BoxSize, GASMASK, NULL, 0, ...) comes next.
 * shq_density_resident / shq_hydro_resident : density() with its Hsml loop (densitytree2.hpp:117-257, treewalk2.h:480-557) and
 *                      hydro_force() (hydratree2.hpp:127-379) for the nlocal targets over the tree of all n; EntVarPred is evaluated
 *                      per particle.  Same kernels as shq_density / shq_hydro_force.
 * shq_gas_get_device : results back into the first n rows of d_rows: which & 1: Hsml, DtHsml, Density, EgyWtDensity,
 *                      DhsmlEgyDensityFactor, DivVel, CurlVel; which & 2: HydroAccel, DtEntropy, MaxSignalVel.
 * Only statistics cross PCIe. */
#define SHQ_GAS_NCOL 28
int shq_gas_set_device(shq_context *ctx, const double *d_rows, int64_t n, int64_t nlocal);
int shq_gas_get_device(shq_context *ctx, double *d_rows, int64_t n, int which);
int shq_density_resident(shq_context *ctx, const shq_density_params *params, shq_sph_stats *stats);
int shq_hydro_resident(shq_context *ctx, const shq_hydro_params *params, shq_sph_stats *stats);

/* For the walk that is open: the export table of its current queue (TopTreeWalk::toptree_visit with cull_node, symmetric
 * for hydro; outputs as shq_ngb_toptree_exports, exportcounts indexed by queue position) and the query records of a
 * table's entries (queries: n records of shq_density_query or shq_hydro_query, whichever walk is open). */
int shq_sph_exports(shq_context *ctx, int32_t *exportcounts, shq_data_index *table, int64_t capacity, int64_t *nexport);
int shq_sph_fill_queries(shq_context *ctx, const shq_data_index *table, int64_t n, void *queries);

/* ---- stellar density ------------------------------------------------------------------------------
 * stellar_density() (libgadget/stellar_density2.cpp:306-341): the SPH volume weight sum(m_j / rho_j [* w_k]) of the gas
 * around each star of `queue` (the reference's StarQueue: build_stellar_density_queue, :285-303; for metal_return it is the
 * queue shq_metal_yields returns), with its own Hsml iteration over ten trial radii per walk (stellareffhsml, ngbiter, postprocess,
 * ngb_narrow_down).  `tree` is the gas tree (GASMASK); gas densities come from the SPH view.  Writes Part[].Hsml of the
 * stars and StarVolumeSPH[PI of the star].  A star with Hsml == 0 is refused (the reference re-seeds it from its father
 * node).  SHQ_ERR_NOCONV beyond MAXITER iterations.  stats->hsml_max_tried is the largest trial radius of any walk of the loop, or
 * any final Hsml: what a sharded caller compares with its ghost halo (shenqi_amd/dist.py:DistMetalReturn.stellar_density). */
typedef struct shq_stellar_params {
    double BoxSize;
    double DesNumNgb;           /* GetNumNgb(GetDensityKernelType()) */
    double MaxNgbDeviation;
    int32_t SPHWeighting;
    int32_t DensityKernelType;
} shq_stellar_params;
int shq_stellar_density(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph,
                        const int32_t *queue, int64_t nqueue, const shq_stellar_params *params, double *StarVolumeSPH,
                        shq_sph_stats *stats);

/* blackhole_veldisp() (libgadget/veldisp2.cpp:164-199): for the active black holes (type 5, not garbage / swallowed) the
 * number of dark-matter particles inside Hsml and the first and second moments of their predicted velocities
 * (DM_VelPred, density2.h:104-111) relative to the hole's, and VDisp = sqrt((V2/N - |V1/N|^2) / 3) where that is positive
 * (BHVelDispOutput::postprocess, :49-63).  `tree` is the dark-matter tree (DMMASK); the particle view needs Vel,
 * FullTreeGravAccel, GravPM, Hsml, TimeBinGravity and PI.  Outputs are indexed by black-hole slot PI; NumDM / V1sumDM /
 * V2sumDM may be NULL; VDisp[PI] is written only where NumDM > 0 and the variance is positive, as the reference does. */
int shq_bh_veldisp(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const int32_t *active, int64_t nactive,
                   const shq_kick_factors *kf, double *NumDM, double (*V1sumDM)[3], double *V2sumDM, double *VDisp);

/* winds_find_vel_disp(), wind part (libgadget/veldisp2.cpp:203-528): for the gas particles of `queue` (the reference's
 * ActiveVDisp from build_vdisp_queue, :376-396, stays on the host: it reads densities and the star-formation threshold) the
 * 1-D velocity dispersion of the ~40 nearest dark-matter particles, found by a density-like loop over five trial radii per
 * walk (NUMDMNGB 40 +- 1), with the Hubble flow hubble * Time^2 * dist in the relative velocity.  `tree` is the dark-matter
 * tree; the particle view needs Vel, FullTreeGravAccel, GravPM, Hsml (the starting DMRadius), TimeBinGravity and PI.
 * VDisp[PI] is written where the reference sets SphP.VDisp (positive variance).  SHQ_ERR_NOCONV beyond MAXITER. */
int shq_wind_veldisp(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const int32_t *queue, int64_t nqueue,
                     const shq_kick_factors *kf, double Time, double hubble, double *VDisp, shq_sph_stats *stats);

/* blackhole_minpot() and the treewalk of blackhole_dynfric() (libgadget/bhdynfric.cpp:44-295, 313-345): for the black holes
 * of `queue` (ActiveBlackHoles / DynFricActive) over the caller's tree (ALLMASK for repositioning; STARMASK + BHMASK, plus
 * DMMASK for BH_DynFrictionMethod > 1, for friction — `typemask` says which types of the tree's particles count):
 *   - the neighbour of lowest Potential inside the hole's Hsml: MinPot / MinPotPos / MinPotVel of slot PI are replaced where it
 *     lies below the value already there (BHReposResult::reduce, :106-118; the caller initialises them as
 *     blackhole_init_potential does, :296-310) and `updated[PI]` is set to 1;
 *   - with method > 0 the friction sums after BHDynFricOutput::postprocess (:66-82): DF_SurroundingDensity (the raw
 *     kernel-weighted mass), DF_SurroundingVel and DF_SurroundingRmsVel normalised where the density is positive.
 * The particle view needs Vel, FullTreeGravAccel, GravPM, Potential, Hsml, TimeBinGravity, Type and PI. */
typedef struct shq_bh_dynfric_out {
    double *MinPot;               /* [nslots], in / out */
    double (*MinPotPos)[3];       /* in / out */
    double (*MinPotVel)[3];       /* in / out */
    int32_t *updated;             /* [nslots] or NULL */
    double *DF_SurroundingDensity; /* out (method > 0), may be NULL */
    double (*DF_SurroundingVel)[3];
    double *DF_SurroundingRmsVel;
} shq_bh_dynfric_out;
int shq_bh_dynfric(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const int32_t *queue, int64_t nqueue,
                   const shq_kick_factors *kf, int BH_DynFrictionMethod, int DensityKernelType, int typemask,
                   const shq_bh_dynfric_out *out);

/* The two legacy-API tree walks of blackhole() (libgadget/blackhole.cpp:217-370), after blackhole_dynfric:
 * symmetric neighbour search over gas + black holes on the caller's tree (GASMASK + BHMASK with hmax: blackhole() calls
 * force_tree_calc_moments when it is missing), one black hole per lane of the SPH operators' wave-collective walk.
 *   shq_bh_accretion   blackhole_accretion_ngbiter / _reduce / _postprocess (:373-692) for the holes of `queue` (ActiveBlackHoles):
 *       BH_SwallowID marks for mergers (r < 2 ForceSoftening / 2.8, the reposition / MergeGravBound rule with check_grav_bound,
 *       the reference's compare-and-swap: the larger ID swallows, an inactive hole can be swallowed by a smaller one);
 *       SPH_SwallowID marks for stochastically swallowed gas (the largest ID + 1 that drew the particle: w = Table[ID % size] <
 *       (BH_Mass - Mass or Mtrack) wk / Density); BH_FeedbackWeightSum, BH_Entropy, BH_SurroundingGasVel, MgasEnc; then Mdot
 *       (Bondi-Hoyle, Eddington cap), BHP.Mass += Mdot dtime, DragAccel, KineticFdbkEnergy / KEflag.  encounter, Mdot, Mass,
 *       DragAccel, KineticFdbkEnergy are written into the slots; the BHPriv arrays into `work` (by slot index, as there).
 *   shq_bh_feedback    blackhole_feedback_ngbiter / _reduce / _postprocess (:728-965) for the holes of `queue` that are not marked
 *       themselves: marked holes and gas are swallowed (Swallowed / slots_mark_garbage, SwallowID, SwallowTime, mass, momentum,
 *       CountProgs), thermal energy into the unswallowed gas inside the kernel (compare-and-swap on the entropy, capped at
 *       MaxThermalU; BHHeated where eeqos[i] != 0) or the released kinetic energy as kicks in the direction get_random_dir draws,
 *       minTimeBin; then BHP.Mass, Part.Vel, Mtrack / Part.Mass and the KineticFdbkEnergy reset.  Particle flags, Vel, Mass, the gas
 *       Entropy and the slots are updated in the caller's arrays.
 * Derived constants are the caller's: EddingtonConst = 4 pi GRAVITY LIGHTCGS PROTONMASS / (0.1 LIGHTCGS^2 THOMPSON) (:379),
 * LightOverUnitVel = LIGHTCGS / UnitVelocity_in_cm_per_s, MaxThermalU = 5e8 / u_to_temp_fac (add_injected_BH_energy, :700-710),
 * Hubble = CP->Hubble, hubble = hubble_function(atime).  The random table is RandTable::Table.  ids[i] = Part[i].ID. */
typedef struct shq_bh_params {
    double BoxSize, ForceSoftening, SeedBHDynMass, atime, a3inv, hubble, GravInternal;
    double BlackHoleAccretionFactor, BlackHoleEddingtonFactor, BlackHoleFeedbackFactor;
    double EddingtonConst, UnitTime_in_s, HubbleParam, LightOverUnitVel, MaxThermalU, OmegaBaryon, Hubble;
    double BHKE_EddingtonThrFactor, BHKE_EddingtonMFactor, BHKE_EddingtonMPivot, BHKE_EddingtonMIndex, BHKE_EffRhoFactor, BHKE_EffCap, BHKE_InjEnergyThr,
        BHKE_SfrCritOverDensity;
    int DensityKernelType, WindsDecoupleSph, RepositionEnabled, MergeGravBound, BH_DRAG, BlackHoleKineticOn;
} shq_bh_params;
typedef struct shq_bh_slot_view {
    void *base;
    size_t elsize;
    int64_t numslots;
    size_t off_mass, off_mdot, off_density, off_mtrack, off_dfaccel, off_vdisp, off_kineticfdbkenergy, off_dragaccel, off_encounter, off_countprogs,
        off_mintimebin, off_swallowid, off_swallowtime;
} shq_bh_slot_view;
typedef struct shq_bh_work {        /* struct BHPriv, blackhole.h:9-45: the caller's arrays, by slot index */
    uint64_t *SPH_SwallowID;        /* [gas slots] */
    uint64_t *BH_SwallowID;         /* [black-hole slots] */
    double *BH_FeedbackWeightSum, *BH_Entropy;
    double (*BH_SurroundingGasVel)[3];
    double *MgasEnc;
    int32_t *KEflag;
    double *BH_accreted_Mass, *BH_accreted_BHMass;   /* feedback only */
    double (*BH_accreted_momentum)[3];
} shq_bh_work;
int shq_bh_accretion(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph, const shq_bh_slot_view *bh,
                     const uint64_t *ids, const int32_t *queue, int64_t nqueue, const shq_kick_factors *kf, const shq_bh_params *params, int64_t Ti_Current,
                     const double *rnd_table, int64_t rnd_size, const shq_bh_work *work);
int shq_bh_feedback(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph, const shq_bh_slot_view *bh,
                    const uint64_t *ids, const int32_t *queue, int64_t nqueue, const shq_kick_factors *kf, const shq_bh_params *params, int64_t MaxPart,
                    const double *rnd_table, int64_t rnd_size, const uint8_t *eeqos, const shq_bh_work *work, int64_t *n_sph_swallowed,
                    int64_t *n_bh_swallowed);

/* The two walks above in the parts a multi-rank driver needs (shenqi_amd/dist.py:DistBlackHole); shq_bh_accretion / shq_bh_feedback
 * stay as they are.  Both walks write on the neighbours' side, and a neighbour may be an import of another rank's particle, so here a
 * walk keeps its hole-side sums and postprocess and only EMITS what it would have written; the records travel to the particle's owner,
 * who applies them per particle in the order of the GLOBAL accretion queue (the ranks' queues one after the other): the serial loop
 * over that queue, deterministic where the one-rank kernels' arrival-order updates of entropy and velocity are not.
 *
 * Rows [0, nlocal) of `parts` are this rank's own, rows >= nlocal imports: ghost_owner[row - nlocal] in [0, nranks) and
 * ghost_index[row - nlocal] >= 0 are the owner's rank and the row there; the queue holds own rows only.  A record is
 * (owner, row at the owner, hole = queue_offset + queue position < 2^31, kind, 8 bytes); an emitted list is sorted by (owner, row, hole),
 * counts[nranks] records per owner, *nrecords their total.  With records == NULL a call only counts (*nrecords set, counts zero, nothing
 * else written); a capacity < *nrecords is SHQ_ERR_INVALID with *nrecords set and nothing else written.
 *
 * shq_bh_accretion_marks   shq_bh_accretion without the two mark arrays: encounter, Mdot, Mass, DragAccel, KineticFdbkEnergy into the
 *     slots and BH_FeedbackWeightSum, BH_Entropy, BH_SurroundingGasVel, MgasEnc, KEflag into `work` for the holes of `queue`.  Emits
 *     kind 0 on a hole (a merger candidate: r < 2 ForceSoftening / 2.8 and the reposition / check_grav_bound flag) and kind 1 on a gas
 *     particle (the draw succeeded), both with bits = the marking hole's ID.
 * shq_bh_marks_resolve     on the owner, the marks gathered from all ranks in any order (it sorts them): zeroes work->SPH_SwallowID
 *     [n_sph_slots] and work->BH_SwallowID[n_bh_slots]; a gas particle gets the largest ID + 1 of its kind-1 marks, a hole the
 *     reference's compare-and-swap rule (blackhole.cpp:570-590) applied to its kind-0 marks in ascending hole order.
 * shq_bh_feedback_effects  shq_bh_feedback for the holes of `queue` whose own mark is 0, the marks in `work` covering the imports'
 *     slots too: accreted mass, BH mass and momentum, CountProgs, minTimeBin, then BHP.Mass, Part.Vel, Mtrack / Part.Mass and the
 *     KineticFdbkEnergy reset of those holes.  Nothing on the neighbours' side; emits kind 0 (the hole is swallowed by this one), kind 1
 *     (the gas particle is), kind 2 (heat: bits = the double injected / mass_j), kind 3 (kick: the double dvel).
 * shq_bh_effects_apply     on the owner, the effects gathered from all ranks in any order: kind 0 SwallowID = BH_SwallowID - 1,
 *     SwallowTime = atime, Swallowed, encounter = 0; kind 1 slots_mark_garbage (ReverseLink = MaxPart + 100); kind 2 BHHeated where
 *     eeqos, add_injected_BH_energy with the MaxThermalU cap; kind 3 Vel += value x get_random_dir(ID).  Before anything is written,
 *     SHQ_ERR_INVALID (shq_bh_marks_resolve too) for a row outside the particles, a kind that does not fit the particle's type, a hole
 *     >= 2^31.
 * Nothing here has run on more than one GPU. */
typedef struct shq_bh_record {
    int32_t owner, part_index;      /* rank that owns the particle, its row there */
    uint32_t hole;                  /* position of the emitting hole in the global queue */
    int32_t kind;
    uint64_t bits;                  /* marks: the hole's ID; effects: a double */
} shq_bh_record;
int shq_bh_accretion_marks(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph, const shq_bh_slot_view *bh,
                           const uint64_t *ids, const int32_t *queue, int64_t nqueue, const shq_kick_factors *kf, const shq_bh_params *params, int64_t Ti_Current,
                           const double *rnd_table, int64_t rnd_size, const shq_bh_work *work, int64_t nlocal, const int32_t *ghost_owner,
                           const int32_t *ghost_index, int nranks, int rank, int64_t queue_offset, shq_bh_record *records, int64_t capacity, int64_t *counts,
                           int64_t *nrecords);
int shq_bh_marks_resolve(shq_context *ctx, const shq_part_view *parts, const uint64_t *ids, const shq_bh_record *marks, int64_t n, int64_t Ti_Current,
                         int64_t n_sph_slots, int64_t n_bh_slots, const shq_bh_work *work);
int shq_bh_feedback_effects(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph, const shq_bh_slot_view *bh,
                            const uint64_t *ids, const int32_t *queue, int64_t nqueue, const shq_kick_factors *kf, const shq_bh_params *params,
                            const double *rnd_table, int64_t rnd_size, const shq_bh_work *work, int64_t nlocal, const int32_t *ghost_owner,
                            const int32_t *ghost_index, int nranks, int rank, int64_t queue_offset, shq_bh_record *records, int64_t capacity, int64_t *counts,
                            int64_t *nrecords);
int shq_bh_effects_apply(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const shq_bh_slot_view *bh, const uint64_t *ids,
                         const shq_bh_record *effects, int64_t n, const shq_bh_params *params, int64_t MaxPart, const double *rnd_table, int64_t rnd_size,
                         const uint8_t *eeqos, const shq_bh_work *work, int64_t *n_sph_swallowed, int64_t *n_bh_swallowed);

/* winds_and_feedback()(libgadget/winds.cpp:295-369): the two asymmetric walks over the gas tree for the new
 * stars of the step — sfr_wind_weight_ngbiter (:411-447: mass of the gas inside the star's Hsml that is not already a wind particle,
 * into TotalWeight[star slot]) and sfr_wind_feedback_ngbiter (:510-565: a gas particle becomes a kick candidate when
 * Table[(star ID + gas ID) % size] < windeff Mass / TotalWeight, with get_wind_params, :489-507) — then the reference's resolution:
 * the candidates sorted by (particle, distance, star ID), the first of every particle kicks (wind_do_kick, :449-471: Vel along
 * get_wind_dir, Entropy += therm / enttou, DelayTime when winds decouple); the results go into the caller's arrays.  WindModel carries the reference's
 * flag bits (WIND_DECOUPLE_SPH 2, WIND_USE_HALO 4, WIND_FIXED_EFFICIENCY 8); the subgrid model (bit 1) does nothing here, as there.
 * `tree` is the gas tree; the star view gives STARP.VDisp (float).  `kicks` (may be NULL) receives the sorted candidate list. */
typedef struct shq_wind_params {
    double BoxSize, Time;
    double WindFreeTravelLength, MaxWindFreeTravelTime, WindEfficiency, WindSpeed, WindSigma0, WindSpeedFactor, MinWindVelocity, WindThermalFactor;
    int WindModel, pad_;
} shq_wind_params;
typedef struct shq_wind_kick {      /* struct StarKick, winds.cpp:175-207 */
    int32_t part_index, pad_;
    double StarDistance;
    uint64_t StarID;
    double StarKickVelocity, StarTherm;
} shq_wind_kick;
typedef struct shq_star_view {
    void *base;
    size_t elsize;
    int64_t numslots;
    size_t off_vdisp;               /* float */
} shq_star_view;
int shq_winds_and_feedback(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph, const shq_star_view *stars,
                           const uint64_t *ids, const int32_t *NewStars, int64_t NumNewStars, const shq_wind_params *params, const double *rnd_table,
                           int64_t rnd_size, double *TotalWeight, shq_wind_kick *kicks, int64_t kicks_capacity, int64_t *nkicks, int64_t *nkicked);
/* The two halves of the call above for a multi-rank driver (shenqi_amd/dist.py:DistWinds): the walks alone — TotalWeight and the sorted
 * candidate list, nothing applied; a candidate's particle may be an imported ghost — and the resolution + kicks for a candidate list
 * gathered from all ranks on the particles' owner (any order: it is sorted again). */
int shq_winds_candidates(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_sph_view *sph, const shq_star_view *stars,
                         const uint64_t *ids, const int32_t *NewStars, int64_t NumNewStars, const shq_wind_params *params, const double *rnd_table,
                         int64_t rnd_size, double *TotalWeight, shq_wind_kick *kicks, int64_t kicks_capacity, int64_t *nkicks);
int shq_winds_apply(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const uint64_t *ids, const shq_wind_kick *kicks, int64_t nk,
                    const shq_wind_params *params, const double *rnd_table, int64_t rnd_size, int64_t *nkicked);

/* The wind model's two particle loops, on the caller's arrays (gas particles of `list`; NULL: all particles, non-gas skipped):
 *   shq_winds_evolve    winds_evolve (winds.cpp:370-387) as cooling_and_starformation calls it per star-forming gas particle: a wind
 *                       particle recouples when its physical density has dropped below WindFreeTravelDensThresh, otherwise its
 *                       DelayTime (capped at MaxWindFreeTravelTime) shrinks by the particle's hydro step dloga_for_bin / hubble.
 *   shq_winds_subgrid   winds_subgrid + winds_make_after_sf (:272-292, 567-585), the subgrid model (WindModel bit 1; a no-op without
 *                       it): gas particle list[k] with stellar mass StellarMasses[k] formed this step is kicked (wind_do_kick) when
 *                       Table[(ID + 2) % size] < 1 - exp(-windeff sm / Mass), with get_wind_params on its SphP.VDisp.  *nkicked counts them.
 * StellarMasses is indexed like the list here (the reference indexes it by slot). */
int shq_winds_evolve(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const int32_t *list, int64_t nlist, double a3inv, double hubble,
                     double WindFreeTravelDensThresh, double MaxWindFreeTravelTime, const shq_kick_factors *kf);
int shq_winds_subgrid(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, size_t sph_off_vdisp, const uint64_t *ids, const int32_t *list,
                      int64_t nlist, const double *StellarMasses, const shq_wind_params *params, const double *rnd_table, int64_t rnd_size, int64_t *nkicked);

/* The treewalk of metal_return() (libgadget/metal_return.cpp:513-530, 573-667), after stellar_density
 * (shq_stellar_density) and with the per-star yields of metal_return_copy (:540-571: the IMF / yield-table integrals, which
 * shq_metal_yields below evaluates on the device): every gas particle inside the kernel of a star of `queue` (r2 > 0, r2 < H^2) receives
 * returnfraction = wk (Mass / Density) / StarVolumeSPH of the star's MassGenerated, MetalGenerated and MetalSpeciesGenerated, unless that
 * would lift it above MaxGasMass: Metals[] (float), Metallicity, Mass (float) and Density are updated with the reference's expressions
 * (:622-660).  The reference serialises the updates of a particle with a spin lock, in whatever order its threads arrive; here the
 * stars reach a particle in queue order (a triple list sorted by particle and queue position, applied by one thread per particle).
 * MassReturn[k] = the mass star queue[k] gave away (metal_return_reduce); the star's own bookkeeping (metal_return_postprocess:
 * Mass -= MassReturn, TotalMassReturned, LastEnrichmentMyr) is shq_metal_return_postprocess below.  All per-star arrays are indexed by
 * queue position. */
typedef struct shq_gas_metal_view {
    void *base;
    size_t elsize;
    int64_t numslots;
    size_t off_density, off_metallicity, off_metals;   /* double, double, float[nmetals] */
    int nmetals, pad_;                                 /* NMETALS = 9 */
} shq_gas_metal_view;
int shq_metal_return(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const shq_gas_metal_view *gas, const int32_t *queue, int64_t nqueue,
                     const double *StarVolumeSPH, const double *MassGenerated, const double *MetalGenerated, const double *MetalSpeciesGenerated /* [nqueue][nmetals] */,
                     double MaxGasMass, int SPHWeighting, int DensityKernelType, double *MassReturn, int64_t *npairs);

/* The parts of the call above for a multi-rank driver (shenqi_amd/dist.py:DistMetalReturn).  Every rank walks its own stars over its own
 * gas plus the gas it imported, sends the triples that fell on imports to the gas's owner, the owner applies all triples of a particle
 * in the order of the GLOBAL queue (the ranks' queues one after the other, in rank order), and the mass each triple moved travels back to the
 * star's rank: the gas ends with the bits of shq_metal_return on the undivided set with that global queue, whatever the decomposition.
 *
 * shq_metal_return_triples  the two emit walks, nothing changed.  Rows [0, nlocal) of `parts` are this rank's own, rows >= nlocal
 *     imports: ghost_owner[row - nlocal] in [0, nranks) and ghost_index[row - nlocal] >= 0 are the owner's rank and the row there.
 *     Every triple becomes (owner, row at the owner, queue_offset + queue position, wk) - own rows: (rank, row) - and the list is sorted by
 *     (owner, row, star): counts[nranks] triples per owner, contiguous, in rank order; *ntriples their total.  With triples == NULL only
 *     counts and *ntriples are returned; a list with capacity < *ntriples is SHQ_ERR_INVALID (counts and *ntriples still set).
 *     queue_offset + nqueue must stay below 2^31 (the star position is 32 bits of a sort key).
 * shq_metal_return_apply    n triples of this rank's own gas, gathered from all ranks in any order (it sorts them by (row, star); owner
 *     is not read): metal_return_ngbiter's body per triple, one thread per gas particle, stars in ascending position.  star_table holds
 *     SHQ_METAL_STAR_NCOL doubles per global queue position: StarVolumeSPH, MassGenerated, MetalGenerated, MetalSpeciesGenerated[9].
 *     Metals, Metallicity, Mass and Density of the touched particles go back into the caller's records; thismass[k] is the mass triple k
 *     moved, 0 where the MaxGasMass rule refused it.  A row outside [0, numpart) or that is not live gas, a star position outside
 *     [0, nstars), or StarVolumeSPH == 0 of a star some triple names: SHQ_ERR_INVALID, nothing written.
 * shq_metal_return_sums     MassReturn[q] for q in [0, nqueue): the thismass of the triples with local queue position qpos == q, added
 *     in ascending (owner, row) order - the same bits on every run. */
#define SHQ_METAL_STAR_NCOL 12
typedef struct shq_metal_triple {
    int32_t owner, part_index;      /* rank that owns the gas particle, its row there */
    uint32_t star;                  /* position in the global queue */
    int32_t pad_;
    double wk;
} shq_metal_triple;
int shq_metal_return_triples(shq_context *ctx, const shq_tree_view *tree, const shq_part_view *parts, const int32_t *queue, int64_t nqueue, int SPHWeighting,
                             int DensityKernelType, int64_t nlocal, const int32_t *ghost_owner, const int32_t *ghost_index, int nranks, int rank,
                             int64_t queue_offset, shq_metal_triple *triples, int64_t capacity, int64_t *counts, int64_t *ntriples);
int shq_metal_return_apply(shq_context *ctx, const shq_part_view *parts, const shq_gas_metal_view *gas, const shq_metal_triple *triples, int64_t n,
                           const double *star_table, int64_t nstars, double MaxGasMass, double *thismass);
int shq_metal_return_sums(shq_context *ctx, const int32_t *qpos, const int32_t *owner, const int32_t *part_index, const double *thismass, int64_t n,
                          int64_t nqueue, double *MassReturn);

/* ---- stellar yields: metal_return_init and the yields of metal_return_copy (libgadget/metal_return.cpp:157-462, 539-569) ------------
 * What metal_return() does per active star before its two tree walks: the star's age, the masses of the stars that die during the
 * step (find_mass_bin_limits), the mass it returns (mass_yield), the maxmassfrac clamp, the queue of the stars with work
 * (metals_haswork) and, for those, the metal and species yields (metal_yield).  The integrals and roots the reference leaves to an
 * adaptive Gauss-Kronrod rule (asked for 1e-4) and a TOMS-748 bracket (asked for 5e-3) are evaluated in closed form:
 * results agree with the reference to its own tolerances, not bit for bit.
 *
 * shq_yields_init uploads the caller's tables once (a second call replaces them; the library ships none) and returns maxmassfrac
 * (:425), evaluated on the host by the routine the kernel uses.  Tables are laid out as libgadget/metal_tables.h has them:
 * value[mass index * nmet + metallicity index]; the species tables are [nmetals][nmass * nmet].  nmetals must be 9 (NMETALS).
 * Requirements (SHQ_ERR_INVALID otherwise): agb_masses[0] >= 1 (only the power-law branch of the Chabrier IMF is integrated),
 * agb_masses[0] <= SNAGBSWITCH <= MAXMASS, increasing axes, and lifetimes that decrease strictly with mass from the first node to
 * the first node at or above MAXMASS, at every metallicity node.
 *
 * The cosmic-time table stands in for atime_to_myr (:170-178): n >= 2 nodes uniform in ln a, a_k = exp(loga0 + k dloga);
 * T[k] = time in Myr since a_0, dTdloga[k] = UnitTime_in_s / SEC_PER_MEGAYEAR / hubble_function(a_k).  Ages are the integral of the
 * cubic Hermite interpolant between ln FormationTime and ln atime. */
typedef struct shq_yield_tables {
    int32_t life_nmet, life_nmass;
    const double *lifetime_metallicity, *lifetime_masses, *lifetime;             /* years */
    int32_t agb_nmet, agb_nmass;
    const double *agb_metallicities, *agb_masses, *agb_total_mass, *agb_total_metals, *agb_yield;
    int32_t snii_nmet, snii_nmass;
    const double *snii_metallicities, *snii_masses, *snii_total_mass, *snii_total_metals, *snii_yield;
    int32_t nmetals, pad_;
    double sn1a_total_metals;
    const double *sn1a_yields;                                                    /* [nmetals] */
} shq_yield_tables;
typedef struct shq_cosmic_time_table {
    int64_t n;
    double loga0, dloga;
    const double *T, *dTdloga;
} shq_cosmic_time_table;
typedef struct shq_yield_params {
    double Sn1aN0, HubbleParam, imf_norm /* compute_imf_norm() */, MAXMASS, SNAGBSWITCH;
} shq_yield_params;
int shq_yields_init(shq_context *ctx, const shq_yield_tables *tables, const shq_cosmic_time_table *times, const shq_yield_params *params,
                    double *maxmassfrac);

/* metal_return_init (:410-462) for the stars (Type 4) of the active list (NULL: all particles; others are skipped), then the queue of
 * metals_haswork (:123-132) in active-list order (a stable compaction: the same list on every run) and metal_return_copy's yields
 * (:539-569) for its stars.  Reads Part.Mass / Type / PI and the star slots; writes, by star slot, StellarAges, LowDyingMass, HighDyingMass
 * and MassReturn (slots of stars not in the list are left alone), LastEnrichmentMyr = age into the slots of the stars the maxmassfrac
 * clamp leaves without work (:445-456; the reference's message() is dropped), and by queue position queue[] (particle indices: the
 * `queue` of shq_stellar_density and shq_metal_return), MassGenerated, MetalGenerated and MetalSpeciesGenerated[][nmetals] (room for as
 * many entries as the active list has).  A FormationTime or atime outside the time table: SHQ_ERR_INVALID, *nbad = the number of such
 * stars (all of the list's stars when it is atime), nothing written.  nbad may be NULL.
 * The particle and slot records are read where the caller keeps them; the context's resident copies are neither used nor changed, so
 * the call can stand anywhere inside a shq_set_inputs_current bracket. */
typedef struct shq_star_yield_view {
    void *base;
    size_t elsize;
    int64_t numslots;
    size_t off_formationtime, off_lastenrichmentmyr;   /* float */
    size_t off_totalmassreturned, off_metallicity;     /* double */
} shq_star_yield_view;
int shq_metal_yields(shq_context *ctx, const shq_part_view *parts, const shq_star_yield_view *stars, const int32_t *active, int64_t nactive, double atime,
                     double *StellarAges, double *LowDyingMass, double *HighDyingMass, double *MassReturn, int32_t *queue, int64_t *nqueue,
                     double *MassGenerated, double *MetalGenerated, double *MetalSpeciesGenerated, int64_t *nbad);
/* metal_return_postprocess (:581-589) for the stars of `queue`: Part.Mass -= MassReturn[k] (float), TotalMassReturned += MassReturn[k],
 * LastEnrichmentMyr = StellarAges[slot] (float).  MassReturn is shq_metal_return's output, by queue position; StellarAges is indexed by
 * star slot.  Where the context holds a copy of these very particles (shq_set_inputs_current), its masses are updated alike. */
int shq_metal_return_postprocess(shq_context *ctx, const shq_part_view *parts, const shq_star_yield_view *stars, const int32_t *queue, int64_t nqueue,
                                 const double *MassReturn, const double *StellarAges);
/* device time of the last shq_metal_yields: ms[0] the first pass (ages, limits, mass return), ms[1] the second (the queue's yields) */
int shq_metal_yields_last_ms(shq_context *ctx, double ms[2]);

/* ---- long-range PM --------------------------------------------------------------------- */

/* Mirror of the PetaPM fields gravpm.cpp reads (libgadget/petapm.h:87-112). */
typedef struct shq_pm_params {
    int32_t Nmesh;
    int32_t pad_;
    double BoxSize;
    double Asmth;
    double G;
} shq_pm_params;

/* One-shot replacement of gravpm_force()'s compute (gravpm.cpp:60-119 minus tree/regions/P(k)):
 * zero GravPM, CIC deposit, r2c, potential_transfer, c2r, readout.  Writes
 * gravpm[numpart][3] and ADDS the PM potential into potential[numpart] (readout_potential,
 * gravpm.cpp:489-491) when potential != NULL.  Particles with the Swallowed flag are skipped
 * (RegionInd = -2, gravpm.cpp:176-178). */
int shq_pm_force(shq_context *ctx, const shq_pm_params *pm, const shq_part_view *parts,
                 double (*gravpm)[3], double *potential);
/* Resident: uses the uploaded particles. */
int shq_pm_run(shq_context *ctx, const shq_pm_params *pm);
int shq_pm_download(shq_context *ctx, double (*gravpm)[3], double *pm_potential);
/* The force part of a PM step as ONE call: gravpm_force, then grav_short_tree for every particle, in the reference's order
 * (libgadget/run.cpp:518-563 — the PM first, because the walk's opening criterion uses FullTreeGravAccel of the last step + the
 * NEW GravPM, gravshort2.hpp:111-121).  Equivalent to shq_pm_run; shq_grav_refresh_oldacc; shq_grav_short_run(all particles,
 * walk_mode = SHQ_WALK_EXACT, optionally | SHQ_WALK_TREE_ORDER) and bit-identical to that sequence.  By default the PM's readout kernel
 * forms OldAcc as it stores GravPM (one pass over the particles instead of two).  With SHQ_TREEPM_FUSE=1 or shq_treepm_set_fuse(ctx, 1),
 * when the walk at hand can carry it (relative criterion, no diagnostic counters, every resident particle a target, mesh below 2^32
 * bytes), the CIC readout and the OldAcc refresh are done by the walk's tasks for their own 64 targets before they walk; that was the
 * default in round 3 and is off since round 4: beside the pair kernel the prologue's loads cost the walk more (2.0 ms) than the two
 * kernels they replace (1.6 ms).  Results land where the separate calls leave them (shq_pm_download, shq_grav_short_download, the
 * resident arrays the kicks read) with the same bits on either route; shq_treepm_last_fused reports which one the last call took. */
int shq_treepm_step(shq_context *ctx, const shq_pm_params *pm, const shq_grav_params *params, int update_potential, int walk_mode);
int shq_treepm_set_fuse(shq_context *ctx, int enable);
int shq_treepm_last_fused(shq_context *ctx, int *fused);
/* gravpm_force started early, for a resident step: the PM of the CURRENT positions (deposit, transforms, readout) is queued on the
 * library's second stream behind everything queued so far, and the call returns; the caller goes on with what needs the positions but
 * not the PM - shq_tree_build - and then calls shq_treepm_step with the same Nmesh, which joins this PM instead of running its own
 * (same results bit for bit).  G > 0: the readout forms OldAcc = |FullTreeGravAccel + GravPM| / G as shq_treepm_step's does.  The
 * reference has no order between force_tree_full and gravpm_force either (run.cpp:476-538; the PM uses no tree).  Every other consumer
 * of PM results (shq_pm_download, shq_kick_pm, ...) joins it too; shq_drift and a particle upload discard it. */
int shq_pm_start(shq_context *ctx, const shq_pm_params *pm, double G);
/* gravpm_force with massive neutrinos (MassiveNuLinRespOn, gravpm.cpp:76-85, 412-435): the PM stops between its forward and inverse
 * halves, where the reference runs its global_analysis hook (compute_neutrino_power, gravpm.cpp:308-321).
 *   shq_pm_forward         : the first half on the resident particles - deposit (honouring the type mask below), forward transform, and
 *                            the raw sums of measure_power_spectrum (as shq_pm_measure_power documents them; shq_pm_download_power returns
 *                            them whatever shq_pm_measure_power is set to).  Queued on the PM's stream as shq_pm_start queues its PM;
 *                            shq_pm_download_power joins it.  The density spectrum stays on the device: the context's PENDING spectrum.
 *   shq_pm_set_mode_factor : table (host, 3 (Nmesh/2)^2 + 1 doubles): T[k2] multiplies every mode of integer k2 of the pending spectrum
 *                            before the Green's function, (v T) green as potential_transfer does with nufac (gravpm.cpp:412-427); T[0] is
 *                            not used (the zero mode is removed).  For the pending spectrum only: the finish consumes it.  NULL clears it;
 *                            a wrong Nmesh is SHQ_ERR_INVALID, no pending spectrum SHQ_ERR_STATE.
 *   finishing              : with a spectrum pending, the next shq_pm_run or shq_treepm_step does not deposit: Green's function x T, inverse
 *                            transform, readout (shq_treepm_step then walks as always).  It wants the forward's params, all four fields, or
 *                            returns SHQ_ERR_STATE.  With shq_pm_measure_power(ctx, 1) it accumulates the P(k) sums of the multiplied
 *                            density (potential_transfer's; scaling Norm by MtotbyMcdm^2, gravpm.cpp:431-435, stays with the caller).
 *   discarded by           : shq_drift, a particle upload, and the other users of the mesh - shq_fft_r2c / c2r, shq_pm_apply, shq_pm_start,
 *                            a slab call of another Nmesh.  The tree walk's mesh scrub (shq_pm_set_mesh_scrub) leaves a pending spectrum alone.
 * The P(k) sums are accumulated with floating-point atomics, as shq_pm_measure_power's: not bit-reproducible.  For the undivided PM; the
 * sharded slab PM splits its X step the same way (shq_pm_slab2_xforward / _xfinish below). */
int shq_pm_forward(shq_context *ctx, const shq_pm_params *pm);
int shq_pm_set_mode_factor(shq_context *ctx, int Nmesh, const double *table);
/* Deposit type mask (hybrid neutrinos: while hybrid_nu_tracer holds, Type 2 is not deposited, gravpm.cpp:84-85, 459-464): bit t set = particles
 * of Type t are deposited; the readout still covers every particle (petapm.cpp:1304-1307).  Default SHQ_ALL_TYPES.  Applies to shq_pm_run,
 * shq_pm_force, shq_pm_start, shq_treepm_step, shq_pm_forward and the slab deposits (shq_pm_slab_deposit, shq_pm_slab2_deposit(_ghosts)).
 * A mask other than all types with particles uploaded without their Type (off_type = SHQ_NOFIELD, or shq_particles_set_device without
 * shq_particles_set_device_types) makes those calls return SHQ_ERR_STATE. */
#define SHQ_ALL_TYPES (-1)
int shq_pm_set_deposit_types(shq_context *ctx, int typemask);
/* Debug / parity taps: copy the mesh after deposit (Nmesh^3 doubles, [x][y][z]) and the
 * potential mesh after c2r. Valid after shq_pm_run with keep_meshes set. */
/* HIP-event durations (ms) of the last shq_pm_run's phases: [0] zero+deposit+convert, [1] r2c,
 * [2] potential transfer, [3] c2r, [4] readout, [5] total. Synchronises. */
int shq_pm_phase_ms(shq_context *ctx, double ms[6]);
/* How the undivided PM runs its five FFT passes (a test / tuning knob; the potential mesh is the same to the bit either way): 1 (default;
 * SHQ_FFT_TRANSPOSED) the mesh changes layout from pass to pass between the mesh and a scratch mesh of the same size, so that one side
 * of every pass moves contiguous 48 KB tiles; 0 in place, column tiles of 64-byte pieces on both sides. */
int shq_pm_set_fft_transposed(shq_context *ctx, int enable);

/* Power spectrum of the PM density, the side product of potential_transfer (measure_power_spectrum /
 * powerspectrum_add_mode, libgadget/gravpm.cpp:323-376, :430).  After shq_pm_measure_power(ctx, 1) every PM
 * run (shq_pm_run / shq_pm_force) also accumulates, per logarithmic k bin (size = Nmesh bins, bin =
 * floor((size-1) / log(sqrt(3) Nmesh / 2) * log(k2) / 2)): power[i] += w |delta_k|^2 / (sinc^2 ...)^2,
 * kk[i] += w |k| (mesh units), nmodes[i] += w, and norm = |delta_0|^2 — the sums pm->ps holds before
 * powerspectrum_sum (powerspectrum.cpp:53-88), which the caller applies (MPI reduction, normalisation, units).
 * Costs one extra pass pair per PM run (the fused X pass never materialises the spectrum), so it is off
 * by default.  The sharded slab PM takes its sums in shq_pm_slab2_xforward / _xfinish (shq_pm_slab_xforward / _xfinish on the torch
 * route): shq_pm_download_power returns this rank's raw sums after either call, for the caller's all-reduce (powerspectrum_sum). */
int shq_pm_measure_power(shq_context *ctx, int enable);
/* the current shq_pm_measure_power setting: 1 on, 0 off, -1 for a null context */
int shq_pm_get_measure_power(shq_context *ctx);
int shq_pm_download_power(shq_context *ctx, int size, double *kk, double *power, int64_t *nmodes, double *norm);
int shq_pm_set_debug(shq_context *ctx, int keep_meshes);
/* The deposit mesh of the NEXT shq_pm_run is cleared in the shadow of the tree walk: the first production-size shq_grav_short_run
 * (exact walk, no diagnostic counters, a task's share <= 64 KB) after a PM run writes the zeros from inside the walk kernel — 3.7 GB
 * at Nmesh 768, spread over the walk's 34 ms on a memory system the walk leaves idle — and that shq_pm_run skips its 0.63 ms
 * clearing kernel (petapm.cpp:1304-1310 deposits into a zeroed mesh either way: results are bit-identical).  The mesh is the
 * library's own buffer and nothing reads it after the readout (shq_pm_set_debug(1) keeps COPIES); any other writer of it
 * (shq_fft_r2c / c2r, a different Nmesh) resets the state.  On by default (SHQ_PM_SCRUB=0 or shq_pm_set_mesh_scrub(ctx, 0) turn it
 * off); shq_pm_mesh_prezeroed reports whether the next shq_pm_run will skip the clearing. */
int shq_pm_set_mesh_scrub(shq_context *ctx, int enable);
int shq_pm_mesh_prezeroed(shq_context *ctx, int *zeroed);
int shq_pm_download_mesh(shq_context *ctx, int which /*0 density,1 potential*/, double *mesh);

/* ---- linear-response massive neutrinos (libgadget/neutrinos_lra.cpp) ----------------------------
 * compute_neutrino_power (gravpm.cpp:308-321: powerspectrum_sum, the square root, delta_nu_from_power) and potential_transfer's nufac
 * table on the device, between shq_pm_forward and the finish.  The state of init_neutrinos_lra is resident: delta_tot[nk][namax],
 * delta_nu_last, delta_nu_init and wavenum live on the device; the host keeps ia, nk and scalefact, which decide every branch.
 * The cosmology stays with the caller: three host callbacks f(a, mi, user) - hubble_function(a), get_omega_nu_nopart(a) and
 * omega_nu_single(a, mi) (mi is 0 for the first two) - called at arguments that do not depend on k, about 10^4 times per step.
 * particle_nu_fraction is closed form from the hybrid parameters below.
 *
 * The time integral of get_delta_nu (:717-725) is not the reference's adaptive rule but a k-independent graded one (csrc/nulra_math.hpp):
 * 8 Gauss-Legendre points per panel, the panels the merged knots of the fs spline and of the history, split so that log(a) - l halves
 * at most per panel, 30 levels into the last interval.  It agrees with a converged sum to a few 1e-11 relative; the reference's rule is
 * run at sqrt(epsilon) = 1.49e-8, so two faithful implementations may differ by that.  While hybrid particle neutrinos gravitate,
 * specialJ is the truncated series, which oscillates as cos(vcrit k fs): the panels are then cut until none spans more than two radians
 * of the largest k's phase, and a step that would need more than 2^20 nodes for that returns SHQ_ERR_INVALID (k and light must be in the
 * same length unit; the reference's rule, at most 2^15 x 61 points, cannot resolve such a phase either).  Three readings of boost are taken without a boost
 * build to check them against:
 *  - makima as stated for the thermal velocities below; Na < 4 history knots use barycentric_rational of order Na - 1, which is the
 *    interpolating polynomial through them;
 *  - gauss_kronrod<double, 61>::integrate defaults to max depth 15 and tolerance sqrt(epsilon);
 *  - boost's splines throw outside their knots.  Here a log k outside the knots of the final spline (and of the rebinning back) takes
 *    the end knot's value - the rule of plane_neutrino_correction_transfer - and a history knot range that does not reach
 *    log(TimeTransfer) continues its end cubic.
 * The sums of a step are reduced in a fixed order without floating-point atomics: two runs from the same sums give the same bits. */
#define SHQ_NULRA_NUSPECIES 3
typedef double (*shq_nulra_cosmo_fn)(double a, int mi, void *user);
typedef struct shq_nulra_params {
    int32_t nk_allocated;       /* init_neutrinos_lra's nk_in: at least the number of non-empty P(k) bins */
    int32_t hybrid_enabled;     /* hybnu.enabled */
    double TimeTransfer, TimeMax; /* namax = ceil((TimeMax - TimeTransfer) / 0.008) + 4 */
    double light, delta_nu_prefac, Omeganonu, OmegaNu1, kBtnu; /* d_tot's fields; OmegaNu1 = get_omega_nu(omnu, 1) */
    double mnu[SHQ_NULRA_NUSPECIES];        /* RhoNuTab[mi].mnu, eV */
    double degeneracy[SHQ_NULRA_NUSPECIES]; /* nu_degeneracies[mi]; a species with 0 is left out */
    double vcrit_by_light, nu_crit_time, nufrac_low[SHQ_NULRA_NUSPECIES]; /* hybnu.vcrit (already divided by light), .nu_crit_time, .nufrac_low */
    double BoxSize_in_MPC;      /* ps->BoxSize_in_MPC */
    int32_t NPowerTable, pad_;  /* the IC transfer table (petaio_read_icnutransfer): logk is log10 k, T_nu = DELTA_NU / DELTA_CB; >= 4 rows, copied */
    const double *logk, *T_nu;
    shq_nulra_cosmo_fn hubble, omega_nu_nopart, omega_nu_single;
    void *user;
} shq_nulra_params;
/* the block petaio_save_neutrinos writes (:267-314): scalefact[ia], delta_tot flat [nk][ia], delta_nu_init[nk], kvalue[nk].
 * delta_nu_last[nk] is this library's addition: with it a restored state continues bit for bit; without it (NULL in set_state, a
 * snapshot of the reference) the first step recomputes it from the history, as the reference does after petaio_read_neutrinos. */
typedef struct shq_nulra_state {
    int32_t ia, nk;
    double *scalefact, *delta_tot, *delta_nu_init, *kvalue, *delta_nu_last;
} shq_nulra_state;
typedef struct shq_nulra_info {
    int32_t ia, nk, nonzero, namax;
    int32_t kept;             /* the last step: 1 its spectrum was saved, 0 discarded (the 0.009 rule), -1 no update */
    int32_t nnodes;           /* quadrature nodes of the last get_delta_nu */
    double nu_prefac;
    double ms[3];             /* device time of the last step: node table upload, delta_nu kernels, mode table */
    double callback_s;        /* host time of the last step's node tables, the callbacks in it */
} shq_nulra_info;
/*   shq_nulra_init       : allocates the state (replacing an earlier one).  The callbacks and `user` must stay valid until shq_nulra_free.
 *   shq_nulra_step       : one delta_nu_from_power at `Time`.  sums == NULL reads the context's own raw P(k) sums, which shq_pm_forward
 *                          just took (nbins is ignored; needs a pending spectrum, SHQ_ERR_STATE otherwise).  Otherwise sums is a DEVICE
 *                          pointer to reduced sums in the layout [nbins] power, [nbins] kk, [nbins] modes (uint64), norm - the caller's
 *                          all-reduce of what shq_pm_download_power returns per rank (a host pointer is taken too: uploaded, and the
 *                          step waits for that copy).  The set of non-empty bins is found once per nbins
 *                          (one download); the first call and the first step after shq_nulra_set_state also wait for the device; every
 *                          other step queues its work behind the forward and returns.  With a spectrum pending the step then fills
 *                          the context's mode-factor table, T[k2] = 1 + nu_prefac spline(log(sqrt(k2) 2 pi / BoxSize_in_MPC)), under the
 *                          rules of shq_pm_set_mode_factor (the finish consumes it; a pending spectrum of an Nmesh other than nbins is
 *                          SHQ_ERR_INVALID).  A second step at the same Time changes no history but refreshes nu_prefac and the table.
 *                          Before shq_nulra_init: SHQ_ERR_STATE.
 *   shq_nulra_mode_table : the table of the last step for any even Nmesh, 3 (Nmesh/2)^2 + 1 doubles to the host; add_one = 0 gives
 *                          nu_prefac * spline alone (the lensing planes', plane.cpp:326-341).  Entry 0 is add_one.
 *   shq_nulra_download   : delta_nu_last[nk], kk[nonzero] (either may be NULL) and the info of the last step.
 *   shq_nulra_delta_nu   : get_delta_nu_combined at scale factor a over the stored history, to the host; changes nothing.
 *   shq_nulra_get_state  : with every pointer NULL fills ia and nk only; otherwise copies the block.  shq_nulra_set_state replaces the
 *                          state; nk > nk_allocated or ia > namax (petaio_read_neutrinos' endrun(5), :404) is SHQ_ERR_INVALID.
 * A NaN in delta_nu_last (endrun(2004), :215) sets a sticky device status: the nulra entry points that follow return SHQ_ERR_DEVICE
 * until shq_nulra_init; the step that produced it may itself still return SHQ_OK, as it does not wait for the device.
 * shq_nulra_host_* is the same engine on the host (csrc/nulra_host.hip: no device, no context); there sums is a host pointer. */
int shq_nulra_init(shq_context *ctx, const shq_nulra_params *params);
int shq_nulra_free(shq_context *ctx);
int shq_nulra_step(shq_context *ctx, double Time, double TimeIC, const void *d_sums, int nbins);
int shq_nulra_mode_table(shq_context *ctx, int Nmesh, int add_one, double *table);
int shq_nulra_download(shq_context *ctx, double *delta_nu_last, double *kk, shq_nulra_info *info);
int shq_nulra_delta_nu(shq_context *ctx, double a, double *delta_nu);
int shq_nulra_get_state(shq_context *ctx, shq_nulra_state *state);
int shq_nulra_set_state(shq_context *ctx, const shq_nulra_state *state);
typedef struct shq_nulra_host shq_nulra_host;
int shq_nulra_host_create(const shq_nulra_params *params, shq_nulra_host **out);
void shq_nulra_host_destroy(shq_nulra_host *h);
int shq_nulra_host_step(shq_nulra_host *h, double Time, double TimeIC, const void *sums, int nbins);
int shq_nulra_host_mode_table(shq_nulra_host *h, int Nmesh, int add_one, double *table);
int shq_nulra_host_download(shq_nulra_host *h, double *delta_nu_last, double *kk, shq_nulra_info *info);
int shq_nulra_host_delta_nu(shq_nulra_host *h, double a, double *delta_nu);
int shq_nulra_host_get_state(shq_nulra_host *h, shq_nulra_state *state);
int shq_nulra_host_set_state(shq_nulra_host *h, const shq_nulra_state *state);

/* ---- slab-sharded PM for multi-GPU runs (one rank per GPU, x-slabs of the mesh) ------------------
 * The mesh is split into slabs of x-planes exactly as petapm splits its real-space pencils over
 * np0 (petapm.cpp:243-257, here np1 = 1).  These are the LOCAL phases on device buffers the
 * caller owns (e.g. torch tensors used for the RCCL exchanges); the exchanges themselves - ghost
 * planes to the neighbours, the all-to-all transposes of the 2-D/1-D FFT stages - are done by the
 * caller with torch.distributed.  See shenqi_amd/dist.py.
 *   deposit : d_mesh_i64 is int64 [nplanes + 1][Nmesh][Nmesh + 2] (last plane = ghost of the right
 *             neighbour; [Nmesh] planes and no ghost when nplanes == Nmesh); zeroed then filled with
 *             the fixed-point CIC deposit of the uploaded particles, all of which must lie in the slab.
 *   green   : potential_transfer on a y-slab of the transposed half spectrum, complex128
 *             [nyl][Nmesh/2 + 1][Nmesh] (x fastest; the reference's Fourier layout, petapm.cpp:258-282).
 *   readout : d_phi_ext is f64 [nplanes + 5][Nmesh][Nmesh + 2], planes plane0-2 .. plane0+nplanes+2
 *             of the potential (periodic); fills the device-resident GravPM / PM potential. */
/* Particle set already in HBM: d_posm = double[n][4] rows (x, y, z, m); the first nlocal rows are this
 * rank's own particles (PM deposit/readout and the default walk targets), the rest imported ghosts
 * that only act as sources in the tree; nlocal == 0 is a rank that owns nothing (no targets, no deposit, no readout).
 * Previous-step accelerations are kept when n is unchanged, and zeroed for every row otherwise.  The tree of the previous set is
 * dropped — a walk before the next shq_tree_build / shq_tree_upload is refused.  flags (any other bit is SHQ_ERR_INVALID):
 *   SHQ_SET_KEEP_TREE   : the caller states that these are the very positions (same count, same order) the current tree was built
 *                         from (a force evaluation repeated on frozen positions): the tree stays.
 *   SHQ_SET_CARRY_LOCAL : a re-import after a drift.  The caller states that the first nlocal rows are the previous set's own
 *                         particles in the same order — moved, with whatever ghosts behind them.  When nlocal equals the previous
 *                         set's, those rows keep FullTreeGravAccel, GravPM, OldAcc, the PM potential and the last walk's results
 *                         whether or not n changed, and only the rows from nlocal on are zeroed.  With another nlocal, or without a
 *                         previous set, the flag has no effect. */
#define SHQ_SET_KEEP_TREE 1
#define SHQ_SET_CARRY_LOCAL 2
int shq_particles_set_device(shq_context *ctx, const void *d_posm, int64_t n, int64_t nlocal, int flags);
/* The Type of every row of that set: d_types_u8 = uint8[n] in device memory, n = the set's row count (else SHQ_ERR_INVALID).  Sets the
 * Type bits of the particle flags and keeps the others; the deposit type mask may then leave types out.  shq_particles_set_device resets
 * every row to Type 1, so a caller issues this again after each set. */
int shq_particles_set_device_types(shq_context *ctx, const void *d_types_u8, int64_t n);
int shq_pm_slab_deposit(shq_context *ctx, const shq_pm_params *pm, int plane0, int nplanes, void *d_mesh_i64);
int shq_pm_slab_green(shq_context *ctx, const shq_pm_params *pm, int y0, int nyl, void *d_spec);
/* green split for a global_analysis hook (massive neutrinos), on the same layout after the caller's X forward:
 *   slab_xforward : zeroes the context's P(k) sums and adds this slab's raw sums of the density (shq_pm_download_power reads them).
 *   slab_xfinish  : table (host, 3 (Nmesh/2)^2 + 1 doubles, NULL for T = 1): (v T) green, potential_transfer's order; with
 *                   shq_pm_measure_power(ctx, 1) the sums are zeroed again and take those of v T. */
int shq_pm_slab_xforward(shq_context *ctx, const shq_pm_params *pm, int y0, int nyl, void *d_spec);
int shq_pm_slab_xfinish(shq_context *ctx, const shq_pm_params *pm, int y0, int nyl, void *d_spec, const double *table);
int shq_pm_slab_readout(shq_context *ctx, const shq_pm_params *pm, int plane0, int nplanes, const void *d_phi_ext);
/* The same phases on the bespoke FFT passes (csrc/fft3d.hip), for mesh sizes that have them
 * (shq_pm_slab_pitch != 0): replaces the 2-D r2c / 1-D FFT / c2r of the slab pipeline (heffte's role in
 * petapm.cpp:281-303) and the separate convert, transpose-to-x-fastest and Green sweeps.  One buffer
 * [nalloc][Nmesh][zp] doubles (zp = shq_pm_slab_pitch, in doubles) is in turn the int64 deposit mesh, the
 * (y, z) half spectrum (complex pitch zp / 2) and the potential; the slab's first own plane is buffer plane
 * `xoff` (2 ghost planes in front, 1 + 3 behind; xoff = 0 and nalloc = Nmesh for a single rank).
 *   slab2_deposit : zero + fixed-point CIC deposit; the plane behind the slab receives the right ghost.
 *   slab2_fft_yz  : direction 0: int64 planes -> half spectrum in (y, z) (in place, `nplanes` planes starting
 *                   at d_planes); direction 1: back to real space.  Unscaled both ways.
 *   slab2_xgreen  : on the y-slab [Nmesh][nyl][zp / 2] the all-to-all delivers (x slowest: the received
 *                   blocks are used as they are), x forward, potential_transfer, x inverse in ONE pass.
 *   slab2_readout : as readout, pitch zp, first own plane at `xoff` of `nalloc` planes. */
int shq_pm_slab_pitch(int Nmesh);
int shq_pm_slab2_deposit(shq_context *ctx, const shq_pm_params *pm, int plane0, int nplanes, int xoff, int nalloc,
                         void *d_mesh_i64);
/* slab2_deposit with `nghost` (1 or 2) planes behind the slab open to the deposit: 2 when the slab also holds the particles of part
 * of its right-hand neighbour's first plane (slabs cut below the plane so that a plane through a cluster's core can be shared:
 * the reference balances at top-leaf granularity, domain.cpp:620-700); slab2_readout then wants 2 + 4 ghost planes (nalloc =
 * nplanes + 6), which its (xoff, nalloc) arguments already express. */
int shq_pm_slab2_deposit_ghosts(shq_context *ctx, const shq_pm_params *pm, int plane0, int nplanes, int xoff, int nalloc, int nghost,
                                void *d_mesh_i64);
int shq_pm_slab2_fft_yz(shq_context *ctx, int Nmesh, void *d_planes, int nplanes, int direction);
/* the same with the pack / unpack of the mesh transposes fused into the Y pass: direction 0 stores the (y, z) spectrum of the planes
 * into d_packed = [nranks][nplanes][Nmesh / nranks][pitch / 2] complex (rows [destination rank][x plane]: the send buffer of the
 * all-to-all), direction 1 starts from d_packed in that layout (what the return all-to-all delivers: rows [source rank][x plane]) */
int shq_pm_slab2_fft_yz_packed(shq_context *ctx, int Nmesh, void *d_planes, int nplanes, int direction, void *d_packed, int nranks);
int shq_pm_slab2_xgreen(shq_context *ctx, const shq_pm_params *pm, void *d_spec, int y0, int nyl);
/* slab2_xgreen in two halves, for a caller with a global_analysis hook (MassiveNuLinRespOn: compute_neutrino_power after
 * powerspectrum_sum's all-reduce, gravpm.cpp:308-321, powerspectrum.cpp:53-88):
 *   slab2_xforward : x forward in place; zeroes the context's P(k) sums and adds this slab's raw sums of the density.  Only the rank
 *                    whose slab holds y = 0 sets Norm; the others leave it 0, so the sum over the ranks is the reference's Norm.
 *   slab2_xfinish  : table (host, 3 (Nmesh/2)^2 + 1 doubles, NULL for T = 1; T[0] is not used): (v T) green, potential_transfer's
 *                    order, then x inverse.  T = 1 does slab2_xgreen's arithmetic: the same bits at Nmesh 48 and 128
 *                    (tests), 2e-15 relative at 768.  With shq_pm_measure_power(ctx, 1) the sums are zeroed
 *                    again and take those of v T (potential_transfer's; scaling Norm by MtotbyMcdm^2 stays with the caller).
 * shq_pm_download_power returns this rank's raw sums after either call; the P(k) sums use floating-point atomics: not bit-reproducible. */
int shq_pm_slab2_xforward(shq_context *ctx, const shq_pm_params *pm, void *d_spec, int y0, int nyl);
int shq_pm_slab2_xfinish(shq_context *ctx, const shq_pm_params *pm, void *d_spec, int y0, int nyl, const double *table);
int shq_pm_slab2_readout(shq_context *ctx, const shq_pm_params *pm, int plane0, int nplanes, int xoff, int nalloc,
                         const void *d_phi);
/* Fixed-point deposit scale 2^e: chosen per context from the local mass sum at particle upload;
 * ranks of one job must agree on it (set it from the global mass sum) so meshes add exactly; e = -1 returns to the
 * per-context choice at the next particle upload. */
int shq_pm_get_deposit_log2scale(shq_context *ctx);
int shq_pm_set_deposit_log2scale(shq_context *ctx, int e);

/* Drop-ins for petapm_fft_r2c / petapm_fft_c2r (libgadget/petapm.cpp:49-71) on one rank: unscaled 3-D transforms of an
 * Nmesh^3 real array ([x][y][z], z fastest: real_space_region, petapm.cpp:256-260) to / from its half spectrum in the
 * reference's Fourier layout [y][z'][x], x fastest, z' <= Nmesh / 2 (fourier_space_region, petapm.cpp:262-270: what
 * pm_apply_transfer_function, :1258-1298, enumerates).  Host pointers.  The _xyz pair keeps the spectrum as [x][y][z'].
 * ONE RANK ONLY (NTask == 1, the 1 x 1 rank grid of petapm.cpp:220-226): for NTask > 1 the reference's 2-D np0 x np1 pencil
 * layouts (petapm.cpp:217-282) are neither produced nor consumed by this library; a multi-rank run replaces petapm_force as a
 * whole with the x-slab pipeline (shq_pm_slab2_* + the caller's all-to-all, INTEGRATION.md "PM on several ranks") — an
 * MI355X-first choice for 8 GPUs on point-to-point xGMI (one transpose pair per PM step instead of ten), not a drop-in for
 * petapm_fft_r2c / c2r there.  The other petapm clients (plane.cpp:326-341, uvbg.cpp:575) get these two calls and nothing more. */
int shq_fft_r2c(shq_context *ctx, int Nmesh, const double *real, double *complx);
int shq_fft_c2r(shq_context *ctx, int Nmesh, const double *complx, double *real);
/* The transfer functions of the other petapm clients: pm_apply_transfer_function (petapm.cpp:1258-1298) followed by
 * petapm_fft_c2r, for one function per call.  Every transfer function of libgenic/zeldovich.cpp:271-321 (density, disp_x/y/z,
 * vel_x/y/z), the lensing planes' neutrino correction (libgadget/plane.cpp:283-304) and the gravity PM's force_x/y/z (gravpm.cpp:464-488)
 * multiplies a mode by  T(k2) x { 1 | i kpos[axis] | i diff_kernel(kpos[axis] 2 pi / Nmesh) }  with T a function of the INTEGER
 * k2 = kx^2 + ky^2 + kz^2 (through |k| = sqrt(k2) 2 pi / BoxSize): the caller tabulates T by k2 with its own functions (DeltaSpec,
 * dlogGrowth, its spline ...), which keeps the values the reference's.  table: host, 3 (Nmesh/2)^2 + 1 entries.
 * zero_mode: what happens to k2 = 0 - 0 the mode is left as it is (the `if(k2)` of the zeldovich transfers), 1 it is set to zero
 * (plane.cpp:286), 2 it is multiplied by T[0] like every other mode (uvbg.cpp:211-215 divide_by_ncell; the reionisation filters
 * filter_pm, uvbg.cpp:218-250, are SHQ_TF_RADIAL tables in k R as well).  complx: [y][z'][x] as shq_fft_r2c returns it; real: [x][y][z], unscaled.  Host pointers; synchronous. */
#define SHQ_TF_RADIAL 0
#define SHQ_TF_GRADIENT 1
#define SHQ_TF_DIFF 2
typedef struct shq_pm_transfer {
    int32_t kind, axis, zero_mode, pad_;
    const double *table;
} shq_pm_transfer;
int shq_pm_apply(shq_context *ctx, int Nmesh, const double *complx, const shq_pm_transfer *tf, double *real);
int shq_fft_r2c_xyz(shq_context *ctx, int Nmesh, const double *real, double *complx);
int shq_fft_c2r_xyz(shq_context *ctx, int Nmesh, const double *complx, double *real);

/* ---- excursion-set reionisation (EXCUR_REION: calculate_uvbg + petapm_reion, libgadget/uvbg.cpp:474-597, petapm.cpp:495-685) ----
 * Mirror of UVBGParams (uvbg.cpp:32-56) plus pm_mass->BoxSize; the mesh is UVBGdim^3. */
typedef struct shq_uvbg_params {
    double ReionRBubbleMax, ReionRBubbleMin, ReionDeltaRFactor;
    int32_t ReionFilterType;     /* 0 real-space top-hat, 1 k-space top-hat, 2 Gaussian (filter_pm, uvbg.cpp:218-250) */
    int32_t RtoMFilterType;      /* 0 top-hat, 1 Gaussian (RtoM, uvbg.cpp:158-176) */
    double ReionGammaHaloBias, ReionNionPhotPerBary, AlphaUV, EscapeFractionNorm, EscapeFractionScaling;
    int32_t ReionUseParticleSFR, pad0_;
    double ReionSFRTimescale;
    int32_t UVBGdim, pad1_;
    double BoxSize;
} shq_uvbg_params;
/* The caller's cosmology and units as values: CP->Omega0, OmegaBaryon, RhoCrit, HubbleParam, hubble_function(CP, Time). */
typedef struct shq_uvbg_cosmo {
    double Time, Omega0, OmegaBaryon, RhoCrit, HubbleParam, hubble;
    double UnitLength_in_cm, UnitMass_in_g, UnitTime_in_s;
} shq_uvbg_cosmo;
/* UVBGgrids' global neutral fractions (uvbg.cpp:424-457) and the number of filter radii the loop ran */
typedef struct shq_uvbg_result {
    double volume_weighted_global_xHI, mass_weighted_global_xHI;
    int32_t nradii, pad_;
} shq_uvbg_result;
/* calculate_uvbg for ONE rank (NTask == 1, as shq_fft_r2c): init_particle_uvbg, the deposit of mass, stellar mass x f_esc (Type 4) and,
 * with ReionUseParticleSFR, Sfr x f_esc (Type 0), one forward transform per field, then for every radius from min(ReionRBubbleMax, BoxSize)
 * down to the cell size the filter, the inverse transforms and reion_loop_pm, and readout_J21.  Several ranks run the same phases on
 * x-slabs of the UVBGdim mesh with the caller's transposes between them: shq_uvbg_slab_* below.
 *   parts     : Pos, Mass and Type (off_type is required); with shq_set_inputs_current(SHQ_CURRENT_PARTICLES) and this very view resident
 *               (uploaded with its Type), the resident positions are read instead.  Every particle in [0, numpart) deposits its mass
 *               (petapm_reion has no regions and no active mask); swallowed particles included.
 *   fesc      : in / out, one per particle: f_esc of the particle's gas or star slot (SphP / StarP EscapeFraction; others are ignored);
 *               on return the transformed value init_particle_uvbg leaves there.
 *   sfr       : SphP.Sfr per particle (read for gas only, and only with ReionUseParticleSFR; may be NULL otherwise).
 *   local_J21 : out, written for gas; zreion: in / out, for gas (1 / Time - 1 where it was -1 and the particle's J21 rises above 0).
 * The deposit is the PM's fixed-point CIC (each field with its own scale 2^(61 - e) from its own sum): the grids do not depend on the
 * particle order.  A negative f_esc after the transform is SHQ_ERR_INVALID before any output is written (the reference ends the run).
 * Changes no state of the context: it stages positions in buffers of its own, which it frees before it returns; the resident particle
 * set, a prestarted PM (shq_pm_start), a pending spectrum (shq_pm_forward), the PM mesh, its scrub state and the deposit scale and type
 * mask all survive the call.  Synchronous. */
int shq_uvbg_calculate(shq_context *ctx, const shq_uvbg_params *params, const shq_uvbg_cosmo *cosmo, const shq_part_view *parts,
                       double *fesc, const double *sfr, double *local_J21, double *zreion, shq_uvbg_result *result);
/* The phases of shq_uvbg_calculate on a rank's x-slab, for several ranks (shenqi_amd/dist.py, DistUVBG; INTEGRATION.md "reionisation on
 * several ranks").  Every d_ pointer is device memory of the caller: d_posm = double[n][4] rows (x, y, z, m) and d_types = uint8[n]
 * Types of the particles whose CIC base cell lies in this rank's planes, d_fesc / d_sfr / d_local_J21 / d_zreion = double[n].
 * A mesh field is one buffer [nalloc][UVBGdim][zp] doubles (zp = shq_uvbg_slab_pitch, 0 for a mesh size without a bespoke transform)
 * that is in turn the int64 deposit, the (y, z) half spectrum and the real mesh of a radius; the window (plane0, nplanes, xoff, nalloc,
 * nghost) is shq_pm_slab2_deposit_ghosts': the slab's first own plane, global plane plane0, is buffer plane xoff, and one plane behind
 * the own ones takes the deposit for the right-hand neighbour (nghost = 1).  One rank is plane0 = 0, xoff = 0, nalloc = UVBGdim.
 * None of the calls reads or writes the PM's state (mesh, deposit scale, type mask, twiddles, pending spectrum).
 *   slab_fesc     : init_particle_uvbg on d_fesc (in / out); sums = this rank's |Mass|, |Mass f_esc| (Type 4), |Sfr f_esc| (Type 0);
 *                   *negative = 1 when a transformed escape fraction is negative (NOT an error here: the ranks must agree first, so
 *                   the caller reduces the flag with the sums and refuses on every rank).  Writes nothing else.  Synchronous.
 *   slab_deposit  : zeroes the two (three with ReionUseParticleSFR) buffers and deposits the fields in ONE particle pass in 64-bit
 *                   fixed point, field f with the scale 2^(61 - exps[f]): exps[f] is the frexp exponent of the field's sum over ALL
 *                   ranks (of 1.0 for a sum of 0), so every rank count deposits the same integers and ghost planes add exactly.
 *                   A particle outside the window is SHQ_ERR_INVALID.  Synchronous.  Without a bespoke transform the pitch of
 *                   the buffers is UVBGdim + 2.
 *   slab_fft_yz   : shq_pm_slab2_fft_yz(_packed) with the scale as an argument: direction 0 takes `nplanes` int64 planes deposited
 *                   with exponent `exp` to their (y, z) half spectrum, direction 1 goes back to real space (exp unused).  d_packed
 *                   (NULL: in place) is shq_pm_slab2_fft_yz_packed's all-to-all buffer.
 *   slab_xforward : X forward of the y-slab [UVBGdim][nyl][zp / 2] complex the all-to-all delivers, in place.  The spectrum stays
 *                   there for the whole radius loop: a radius costs one all-to-all per field.
 *   slab_tables   : the filter tables (shq_uvbg_filter_table, host) of radii[0 .. nradii - 2], kept on the device until the next call;
 *                   the last radius is the unfiltered step.  Every rank makes the same tables.
 *   slab_xfilter  : radius r of those tables on the kept spectrum d_spec: every mode (v / ncell) T[k2] - divide_by_ncell, then
 *                   filter_pm, k2 from the signed (kx, ky = y0 + row, kz) - then the X inverse, stored OUT OF PLACE into d_out (same
 *                   shape: what the return all-to-all sends).  d_spec is only read.
 *   slab_filter   : the same factor for a mesh size without a bespoke transform, between the caller's own X transforms: d_spec =
 *                   [UVBGdim][nyl][UVBGdim / 2 + 1] complex, dense, x slowest, into d_out of that shape (may be d_spec).
 *   slab_cells    : reion_loop_pm of radius R over the nplanes own planes of the real meshes (pitch zp, from buffer plane xoff) and of
 *                   the rank's dense float planes d_J21 / d_xHI [nplanes][UVBGdim][UVBGdim] (J21 = 0, xHI = 1 before the first
 *                   radius).  last != 0: the unfiltered step; sums then takes this rank's sums of xHI, xHI density_over_mean and
 *                   density_over_mean, from a fixed grid: two runs agree bit for bit (synchronous then).
 *   slab_readout  : readout_J21 for this rank's gas: d_J21 = float [nalloc][UVBGdim][UVBGdim], the own planes and behind them the
 *                   right-hand neighbour's first plane (nalloc = nplanes + 1; nplanes = UVBGdim: the periodic grid, nalloc = UVBGdim).
 *                   Writes d_local_J21 / d_zreion of gas.  Synchronous. */
int shq_uvbg_slab_pitch(int UVBGdim);
int shq_uvbg_slab_fesc(shq_context *ctx, const shq_uvbg_params *params, const shq_uvbg_cosmo *cosmo, const void *d_posm, const void *d_types,
                       int64_t n, void *d_fesc, const void *d_sfr, double sums[3], int *negative);
int shq_uvbg_slab_deposit(shq_context *ctx, const shq_uvbg_params *params, const void *d_posm, const void *d_types, int64_t n,
                          const void *d_fesc, const void *d_sfr, const int exps[3], int plane0, int nplanes, int xoff, int nalloc, int nghost,
                          void *d_m0, void *d_m1, void *d_m2);
int shq_uvbg_slab_fft_yz(shq_context *ctx, int UVBGdim, void *d_planes, int nplanes, int direction, int exp, void *d_packed, int nranks);
int shq_uvbg_slab_xforward(shq_context *ctx, int UVBGdim, void *d_spec, int y0, int nyl);
int shq_uvbg_slab_tables(shq_context *ctx, int filter_type, int UVBGdim, double BoxSize, const double *radii, int nradii);
int shq_uvbg_slab_xfilter(shq_context *ctx, int UVBGdim, const void *d_spec, void *d_out, int y0, int nyl, int r);
int shq_uvbg_slab_filter(shq_context *ctx, int UVBGdim, const void *d_spec, void *d_out, int y0, int nyl, int r);
int shq_uvbg_slab_cells(shq_context *ctx, const shq_uvbg_params *params, const shq_uvbg_cosmo *cosmo, double R, int last, const void *d_mass,
                        const void *d_star, const void *d_sfr, int zp, int xoff, int nplanes, void *d_J21, void *d_xHI, double sums[3]);
int shq_uvbg_slab_readout(shq_context *ctx, const shq_uvbg_params *params, const shq_uvbg_cosmo *cosmo, const void *d_posm, const void *d_types,
                          int64_t n, const void *d_J21, int plane0, int nplanes, int nalloc, void *d_local_J21, void *d_zreion);
/* save_uvbg_grids' data: with shq_uvbg_keep_grids(ctx, 1) every later call copies its J21 and xHI grids to host memory of the context
 * (2 x 4 Nmesh^3 bytes); shq_uvbg_download_grids returns the last call's as dense [x][y][z] float (SHQ_ERR_STATE without one, SHQ_ERR_INVALID
 * for another Nmesh).  keep_grids(ctx, 0) frees them. */
int shq_uvbg_keep_grids(shq_context *ctx, int enable);
int shq_uvbg_download_grids(shq_context *ctx, int Nmesh, float *J21, float *xHI);
/* HIP-event durations (ms) of the last call: [0] f_esc, deposit and forward transforms, [1] the radius loop, [2] readout, [3] all of it
 * on the device (uploads and downloads included). */
int shq_uvbg_phase_ms(shq_context *ctx, double ms[4]);
/* Host only: filter_pm's factor (uvbg.cpp:218-250) per integer k2 = 0 .. 3 (Nmesh/2)^2 into table (3 (Nmesh/2)^2 + 1 doubles), with the
 * reference's expressions and libm calls (sinf / cosf / powf in float for the real-space top-hat, pow(M_E, .) for the Gaussian). */
int shq_uvbg_filter_table(int filter_type, int Nmesh, double BoxSize, double R, double *table);

/* ---- helium reionisation by quasar bubbles (do_heiii_reionization / turn_on_quasars, libgadget/cooling_qso_lightup.cpp:225-617) ----
 * HeIIIionized is bit 2 of the particle flag byte (after IsGarbage and Swallowed, before BHHeated); the context's copy of the flags keeps
 * it in the same bit. */
#define SHQ_FLAG_HEIII 4u
typedef struct shq_heiii_params {
    double BoxSize, atime;
    double qso_candidate_min_mass, qso_candidate_max_mass, mean_bubble, var_bubble, heIIIreion_finish_frac;   /* QSOLightupParams */
    double desired_ion_frac;      /* (*HeIII_intp)(atime): the history table and its interpolation stay with the caller */
    double qso_inst_heating;      /* Q_inst of the history file, erg */
    double uu_in_cgs;             /* UnitInternalEnergy_in_cgs */
    double OmegaBaryon, HubbleParam;
    double CurrentParticleOffset[3];
    int64_t n_gas_tot;            /* SlotsManager->info[0].size */
} shq_heiii_params;
typedef struct shq_heiii_quasar { /* one FdHelium line (:574-583) */
    int32_t group, pad_;          /* catalogue index of the lit group, -1 for a draw that lit nothing (position 0, or off the list) */
    double pos[3];                /* CM - CurrentParticleOffset wrapped into (0, BoxSize]; zeros when group == -1 */
    double ionfrac;               /* curionfrac after this quasar */
    int64_t n_ionized;
} shq_heiii_quasar;
typedef struct shq_heiii_result {
    double init_ionfrac, final_ionfrac;
    int64_t n_candidates;         /* candidate groups built (0 when the box was already ionised enough) */
    int64_t n_iterations;         /* iterations of the quasar loop = FdHelium lines */
    int64_t n_flash;              /* particles flash-ionised (desired > heIIIreion_finish_frac) */
    int64_t n_ionized;            /* particles ionised by quasar bubbles (tot_n_ionized) */
} shq_heiii_result;
/* turn_on_quasars for ONE rank.  Candidates are the groups of the RESIDENT FOF catalogue (shq_fof; SHQ_ERR_STATE without one) with
 * min <= Mass <= max, in catalogue order; TotNgroups is the catalogue's length.  The catalogue is read before anything is uploaded.
 *   parts / sph : Pos, Type, PI, the flag byte, and what shq_sph_state_upload needs (Hsml, Vel); Density and Entropy through PI.  Uploaded
 *                 or skipped under shq_set_inputs_current as every one-shot operator.  Every gas particle needs a PI inside the slot array.
 *   gas_tree    : the gas tree (GASMASK | BHMASK, with father) — required when var_bubble > 0 (SHQ_ERR_INVALID without it), where a negative
 *                 radius makes membership depend on the tree; may be NULL otherwise (and is then not uploaded).
 *   rnd_table   : RandTable::Table (rnd_size entries), read on the host only.
 *   log         : FdHelium lines, log_capacity of them at most (may be NULL); *nlog = n_iterations.
 * Ionised particles get flag |= SHQ_FLAG_HEIII and Entropy += deltau / uu_in_cgs / entropytou in the caller's records and in the context's
 * copies; nothing else is written.  The quasar draws and radii are made on the host with glibc's libm, the bubbles are swept on the
 * device in batches (DESIGN.md §"Helium reionisation").  Synchronous. */
int shq_heiii_reionization(shq_context *ctx, const shq_heiii_params *params, const shq_part_view *parts, const shq_sph_view *sph,
                           const shq_tree_view *gas_tree, const double *rnd_table, int64_t rnd_size, shq_heiii_quasar *log,
                           int64_t log_capacity, int64_t *nlog, shq_heiii_result *result);
/* What the last shq_heiii_reionization did on the device: HIP-event times (ms) of [0] the uploads and the eligible list, [1] the sweeps,
 * [2] the stop replays, applies and compactions, [3] the whole call; the number of sweeps, the draws and the lit bubbles they covered, the
 * eligible particles the first sweep tested, and the particle-bubble tests all sweeps made (eligible x lit, summed per sweep); per sweep (the
 * first SHQ_HEIII_NSTAT) its draws, lit bubbles and eligible particles. */
#define SHQ_HEIII_NSTAT 32
typedef struct shq_heiii_stats {
    double ms[4];
    int64_t nsweeps, ndraws, nbubbles, neligible, ntests;
    int32_t sweep_draws[SHQ_HEIII_NSTAT], sweep_lit[SHQ_HEIII_NSTAT];
    int64_t sweep_eligible[SHQ_HEIII_NSTAT];
} shq_heiii_stats;
int shq_heiii_last_stats(shq_context *ctx, shq_heiii_stats *stats);

/* ---- the same operator in phases, for a driver that runs turn_on_quasars over several ranks (shenqi_amd/dist.py:DistHeIII) ----
 * On several ranks every rank holds some of the gas and some of the groups; the bubble of a lit quasar reaches gas on every rank, and the
 * loop's control needs the per-bubble counts summed over the ranks.  So the one call above is cut where those sums are taken:
 *   open   : upload (or reuse), flash, count, build the list of eligible gas (Type 0, not garbage, not ionised) as records (x, y, z, index)
 *   sweep  : every eligible record gets the seq of the FIRST bubble of the list that holds it; hits are counted per seq
 *   commit : the records whose first hit has seq < seq_stop are flagged and heated and leave the eligible list
 *   close  : flag bit and Entropy of everything ionised since open go into the caller's records; the run is freed
 * sweep and commit alternate any number of times between open and close (a sweep may be repeated; a commit needs a sweep since the last
 * commit).  The run lives in the context; one run at a time, and not while an SPH walk is open.  A call out of order returns SHQ_ERR_STATE.
 * Between open and close the context's particles and gas state belong to the run: the eligible records hold particle indices, and the
 * heating lives in the context's copies.  What is checked: shq_density_open and shq_hydro_open refuse while a run is open, and every
 * phase returns SHQ_ERR_STATE when the context's particle count is no longer the one at open.  What is not: an upload of another set of
 * the same length, or a one-shot operator on the context, between open and close; the caller must not make one.  Positions are finite
 * (shq_particles_upload refuses others), so the extents are those of every eligible record.
 * Nothing is written to the caller's records before close, so a failed
 * call leaves them untouched, and after a failed sweep or commit the run can still be closed.  Membership is the particle test of the
 * legacy walk, !(r2 > R*R) with r2 summed in x, y, z order of NEAREST(c - Pos): that decides alone for R >= 0, +inf and NaN on any number
 * of ranks.  For R < 0 (-inf included) the walk's node test decides too, and with it each rank's tree: the sweep refuses such a radius
 * (SHQ_ERR_INVALID); negative radii stay with shq_heiii_reionization and its gas tree. */
typedef struct shq_heiii_bubble {
    double c[3];                  /* the quasar's CM */
    double R;                     /* bubble radius: >= 0, +inf or NaN */
    int32_t seq, pad_;            /* the bubble's number: strictly increasing along the list, 0 <= seq < nseq */
} shq_heiii_bubble;
#define SHQ_HEIII_MAX_SEQ 1024
/* params as for the one call (the mass window, var_bubble and the offset are not read).  n_flash: particles flash-ionised by this call;
 * n_ionized_now: Type-0 particles with the flag after the flash, garbage included (gas_ionization_fraction's local count); n_eligible:
 * length of the eligible list; lo / hi: per axis the smallest and largest coordinate of the eligible records (a two-pass min / max
 * reduction: the same bits on every run), lo = +inf > hi = -inf when there is none. */
int shq_heiii_open(shq_context *ctx, const shq_heiii_params *params, const shq_part_view *parts, const shq_sph_view *sph, int64_t *n_flash,
                   int64_t *n_ionized_now, int64_t *n_eligible, double lo[3], double hi[3]);
/* counts[nseq] (host, u64): hits per seq, 0 for every seq not in the list.  nbubbles == 0 is valid (all zeros; bubbles may be NULL).
 * SHQ_ERR_INVALID for nseq outside 1 .. SHQ_HEIII_MAX_SEQ, a seq that does not increase or is not below nseq, or a radius < 0. */
int shq_heiii_sweep(shq_context *ctx, const shq_heiii_bubble *bubbles, int nbubbles, int nseq, uint64_t *counts);
/* seq_stop == 0 commits nothing; n_committed may be NULL */
int shq_heiii_commit(shq_context *ctx, int seq_stop, int64_t *n_committed);
/* parts / sph: the records given to open (the same numpart; SHQ_ERR_INVALID and the run stays open otherwise).  n_rows (may be NULL):
 * particles written = flashed + committed.  The run is freed whether or not the download succeeds.  shq_heiii_last_stats then holds the
 * run's numbers: ms = open, sweeps, commits, and those three plus close; nsweeps, nbubbles, neligible, ntests as above; ndraws = 0. */
int shq_heiii_close(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, int64_t *n_rows);
/* Host only: the numbers of the loop that must be glibc's, from the functions shq_heiii_reionization itself uses.  radii_out[i] =
 * gaussian_rng(mean_bubble, sqrt(var_bubble), minids[i]) (:249-255); *non_overlapping_bubble_number as :514-518 forms it from
 * n_gas_tot, mean_bubble, OmegaBaryon, HubbleParam and atime.  minids / radii_out may be NULL with n == 0. */
int shq_heiii_host_numbers(const shq_heiii_params *params, const uint64_t *minids, int64_t n, const double *rnd_table, int64_t rnd_size,
                           double *radii_out, int64_t *non_overlapping_bubble_number);

/* ---- lensing potential planes (write_plane's compute, libgadget/plane.cpp:511-600; cutPlaneGaussianGrid and
 * calculate_lensing_potential, lenstools.cpp:168-319; the PM neutrino correction, plane.cpp:355-475) ----
 * For ONE rank: the caller sums the planes over ranks (MPI_Reduce) as write_plane does. */
typedef struct shq_lens_params {
    int32_t Resolution;           /* PlaneResolution, 2 .. 46340 */
    int32_t ncuts, nnormals;      /* ncuts == 0: write_plane's default list (plane.cpp:524-530), (0.5 + i) Thickness for
                                     i < (size_t)(BoxSize / Thickness) (shq_lens_num_cuts) */
    int32_t exclude_type2;        /* hybrid_nu_tracer(CP, atime): Type 2 particles are skipped */
    const double *CutPoints;      /* ncuts, internal length units */
    const int32_t *Normals;       /* nnormals, each 0..2 (repeats allowed, as BuildOutputList allows) */
    double Thickness;             /* <= 0: BoxSize (plane.cpp:519-522) */
    double BoxSize;
    double CurrentParticleOffset[3];
} shq_lens_params;
typedef struct shq_lens_cosmo {
    double atime, comoving_distance, HubbleParam;
    double omega_source;          /* Omega0 - a^3 Omega_nu_nopart under MassiveNuLinRespOn (lenstools_particle_omega_source); > 0 */
    int64_t num_particles_tot;    /* global active count (the sum of shq_lens_count_active over ranks); > 0 */
} shq_lens_cosmo;
typedef struct shq_lens_numesh {  /* the optional PM neutrino correction (cutPlanePMNeutrinoCorrection) */
    int32_t Nmesh, x0, nx, pad_;  /* this rank holds mesh planes [x0, x0 + nx) */
    double inv_fft_norm, mean_mass_cell;
    const double *real;           /* host, dense [nx][Nmesh][Nmesh] as shq_pm_apply returns it (unscaled) */
} shq_lens_numesh;
/* lenstools_particle_is_active's count on this rank: not Swallowed, and not Type 2 under exclude_type2 (garbage particles count). */
int shq_lens_count_active(shq_context *ctx, const shq_part_view *parts, int exclude_type2, int64_t *count);
/* The number of cuts a call makes: ncuts, or the default list's length when ncuts == 0. */
int shq_lens_num_cuts(const shq_lens_params *params, int32_t *ncuts);
/* Every (cut, normal) plane of write_plane in one call:
 *   parts  : Pos, Type and the flag word (Mass is not read: the reference counts particles).  With shq_set_inputs_current(
 *            SHQ_CURRENT_PARTICLES) and this very view resident (uploaded with Type and the flag word), the resident positions, types
 *            and flags are read and nothing is uploaded.
 *   nu     : the rank's x-slab of the PM neutrino correction mesh, or NULL for none.  Its projection is indexed
 *            [global[(normal + 1) % 3]][global[(normal + 2) % 3]]: for normal 1 that is [z][x], the transpose of the particle plane's
 *            [x][z], as in the reference.
 *   planes : out [ncuts][nnormals][R][R], the potential planes of this rank (particle plane layout: normal 0 [y][z], 1 [x][z], 2 [x][y]).
 *   num_particles_plane : out [ncuts][nnormals]; counts : optional out [ncuts][nnormals][R][R] NGP counts (NULL skips them).
 * SHQ_ERR_INVALID before anything is written for a normal outside 0..2, Resolution < 2, num_particles_tot <= 0, omega_source <= 0, a
 * correction with a bad Nmesh, x0 or nx, non-finite BoxSize / Thickness / cut points / offsets, or 2^32 particles or more.  The particles
 * are read once per call; the correction mesh once per distinct normal (for up to 8 cuts).  Changes no state of the context: the
 * resident set, a prestarted PM, a pending spectrum, the PM mesh, its scrub state and the deposit type mask survive.  Synchronous. */
int shq_lens_planes(shq_context *ctx, const shq_lens_params *params, const shq_lens_cosmo *cosmo, const shq_part_view *parts,
                    const shq_lens_numesh *nu, double *planes, int64_t *num_particles_plane, uint32_t *counts);
/* HIP-event durations (ms) of the last shq_lens_planes: [0] particle staging and binning, [1] the particle planes' 2-D solves, [2] the
 * correction (mesh upload, projection, solve, bilinear add), [3] all of it on the device, downloads included. */
int shq_lens_phase_ms(shq_context *ctx, double ms[4]);

/* ---- Zel'dovich displacements (displacement_fields, libgenic/zeldovich.cpp:150-264; gaussian_fill / pmic_fill_gaussian_gadget,
 * zeldovich.cpp:362-383 and libgenic/pmesh.h:64-178; the transfers of zeldovich.cpp:277-334) ----  one rank.
 * The Gaussian field of (Nmesh, Seed, UnitaryAmplitude, InvertPhase) is filled on the device and stays resident in the context: the
 * reference fills the same field once per species (genic/main.cpp).  It is discarded by a fill or a displacement call with another key,
 * by shq_zeldovich_drop_field and by shq_shutdown, and by nothing else. */
typedef struct shq_zeldovich_params {
    int32_t Nmesh;               /* even, 4 .. 2048 */
    int32_t Seed;                /* GenicConfig.Seed */
    int32_t UnitaryAmplitude, InvertPhase;
    int32_t ScaleDepVelocity;    /* PowerP.ScaleDepVelocity: VelX/Y/Z from dlogGrowth; otherwise Vel = Disp */
    int32_t pad_;
    double BoxSize;
    double vel_prefac;           /* as zeldovich.cpp:195-208 forms it from hubble_function, F_Omega and UsePeculiarVelocity */
} shq_zeldovich_params;
/* Host only: the seed tables [0][0] and [1][1] of pmesh.h:74-90 on one rank (mt19937(Seed), one 32-bit draw per SETSEED,
 * seed = (unsigned)(0x7fffffff * draw / 2^32), the reference's write order), Nmesh^2 entries each, index i * Nmesh + j. */
int shq_zeldovich_seed_table(int Nmesh, int Seed, uint32_t *table00, uint32_t *table11);
/* Host only: the factors of density_transfer and disp_transfer by integer k2 (3 (Nmesh/2)^2 + 1 entries, entry 0 is 0) from the
 * caller's delta[k2] = DeltaSpec(kmag, ptype) and growth[k2] = dlogGrowth(kmag, ptype), kmag = sqrt(k2) 2 pi / BoxSize:
 *   dens_fac = exp(-k2 / Nmesh^2) delta / sqrt(BoxSize^3)     (SHQ_TF_RADIAL, zero_mode 0 for shq_pm_apply)
 *   disp_fac = 1 / (2 pi) / sqrt(BoxSize) / k2 * delta         (SHQ_TF_GRADIENT)
 *   vel_fac  = the same with growth instead of delta            (SHQ_TF_GRADIENT; NULL skips it, as does growth == NULL)
 * glibc's exp and sqrt.  shq_zeldovich_displacements forms its gradient factor per mode in the reference's order,
 * 1 / (2 pi) / sqrt(BoxSize) * kaxis / k2 * delta, which differs from disp_fac * kaxis in the last bit. */
int shq_zeldovich_factor_tables(int Nmesh, double BoxSize, const double *delta, const double *growth, double *dens_fac, double *disp_fac,
                                double *vel_fac);
/* Fill the resident field now (a displacement call does it when it finds none with its key). */
int shq_zeldovich_fill(shq_context *ctx, int Nmesh, int Seed, int UnitaryAmplitude, int InvertPhase);
/* Debug: the resident field to the host in the reference's Fourier layout [y][z'][x] (as shq_fft_r2c returns a spectrum and shq_pm_apply
 * takes one), Nmesh^2 (Nmesh/2 + 1) complex.  SHQ_ERR_STATE without a resident field. */
int shq_zeldovich_download_field(shq_context *ctx, int Nmesh, double *complx);
/* Free the resident field. */
int shq_zeldovich_drop_field(shq_context *ctx);
/* Debug: columns per launch of the fill (rounded up to 64; 0 restores the default).  The field does not depend on it. */
int shq_zeldovich_set_fill_chunk(shq_context *ctx, int64_t ncolumns);
/* displacement_fields in one call:
 *   delta, growth : host tables by k2 as above; growth may be NULL without ScaleDepVelocity
 *   pos           : host [n][3], the undisplaced positions, each in [0, BoxSize)
 *   pos_out       : out [n][3], Pos + Disp after periodic_wrap (may be pos itself)
 *   vel           : out [n][3];  density : out [n];  disp : out [n][3] or NULL
 *   maxdisp       : the largest signed Disp component, from 0;  maxvel : the largest |Vel|^2 (the reference prints its root)
 * SHQ_ERR_INVALID before anything is written for an odd Nmesh or one outside 4 .. 2048, a BoxSize that is not finite and > 0, a position
 * outside [0, BoxSize) (the reference ends the run: "particle out of cell"), a non-finite table entry, or ScaleDepVelocity with
 * growth == NULL.  The call owns its work mesh and particle buffers: the resident particle set and tree, the PM mesh and its result, a
 * pending spectrum and the deposit type mask survive.  A prestarted PM is joined first, because the transforms share the context's
 * twiddle table with it.  Of the context only the resident field and that table change.  Synchronous. */
int shq_zeldovich_displacements(shq_context *ctx, const shq_zeldovich_params *params, const double *delta, const double *growth, int64_t n,
                                const double *pos, double *pos_out, double *vel, double *density, double *disp, double *maxdisp,
                                double *maxvel);
/* HIP-event durations (ms) of the last shq_zeldovich_displacements: [0] the fill (exactly 0 when the resident field was reused), [1] the
 * uploads, transfers, transforms and readouts, [2] the particle loop, [3] all of it on the device, downloads included. */
int shq_zeldovich_phase_ms(shq_context *ctx, double ms[4]);
/* Test entry for the sampler: n generators, each seeded with seeds[t] (init_genrand) or, with states != NULL, started from the 624 words
 * states[t] as they are before their first twist.  raw: out [n][m], the first m 32-bit outputs.  pairs: out [n][m/2][2], the first m/2
 * SAMPLEs (pmesh.h:55-62) of the same start as (phase, ampl before the log), the ampl == 0 redraw included.  m even, n <= 65536. */
int shq_zeldovich_column_draws(shq_context *ctx, int n, const uint32_t *seeds, const uint32_t *states, int m, uint32_t *raw, double *pairs);

/* ---- Zel'dovich displacements on several ranks (shenqi_amd/dist.py, DistZeldovich): the phases of shq_zeldovich_displacements as
 * entry points of their own, with the caller's exchanges between them.  The reference gives every task its sub-block of the lattice
 * (zeldovich.cpp:46-65), fills only its own Fourier region (pmesh.h:93-172) and all-reduces the two maxima (zeldovich.cpp:150-264).
 *
 * Every pointer named d_ is DEVICE memory of the caller; nothing is uploaded or downloaded but the tables and the two maxima.  The
 * Gaussian field lives on the rank's y-slab, the mesh rows y0 <= y < y0 + nyl: d_spec = [Nmesh][nyl][zpc] complex, x slowest, zpc =
 * shq_zeldovich_slab_pitch(Nmesh) / 2 - or, for a mesh size without a bespoke transform (pitch 0), dense with Nmesh / 2 + 1.  One mt19937
 * per mesh column means a rank makes exactly its own columns: the slab's modes are the SAME BITS as the matching rows of
 * shq_zeldovich_download_field, whatever the slab.  A field's real mesh lives on the rank's x planes, [nalloc][Nmesh][zp] doubles.
 * None of these calls reads or writes the PM's state (mesh, deposit scale, type mask, twiddles, pending spectrum, prestarted PM) or
 * the one-rank resident field: twiddles, tables and flags are the family's own.  They run on the context's stream; fill, tables,
 * gather and finalize return synchronised, xtransfer, transfer and fft_yz only launch.
 *
 * The order of a call, per rank:
 *   shq_zeldovich_slab_fill       once per (Nmesh, Seed, flags): d_spec is only read afterwards, so it serves every field and species;
 *                                 pad columns z' > Nmesh / 2 are written as 0; chunked by shq_zeldovich_set_fill_chunk
 *   shq_zeldovich_slab_tables     dens[k2] made on the host as the one-rank call makes it, delta[k2], growth[k2] (NULL: no velocity
 *                                 fields) uploaded; they stay on the device until the next call.  SHQ_ERR_INVALID for a bad mesh size,
 *                                 a BoxSize that is not finite and > 0, or a non-finite entry
 *   per field 0 .. 6 (Density, DispX/Y/Z, VelX/Y/Z):
 *     shq_zeldovich_slab_xtransfer  the transfer function per mode (the one-rank kernel's arithmetic, signed kx, ky = y0 + row, kz;
 *                                 k2 = 0 left as it is) fused into the X inverse, stored OUT OF PLACE into d_out of d_spec's shape:
 *                                 the buffer of the return all-to-all.  SHQ_ERR_STATE without tables of this Nmesh and BoxSize
 *     (shq_zeldovich_slab_transfer  the factor alone on the dense slab, between the caller's own X transforms, for a mesh size without
 *                                 a bespoke transform; d_out may be d_spec)
 *     shq_zeldovich_slab_fft_yz   the Y/Z inverse of the x planes, the Y pass reading the all-to-all buffer d_packed =
 *                                 [nranks][nplanes][Nmesh / nranks][zpc] (NULL: the planes hold the spectrum already)
 *     shq_zeldovich_slab_gather   pm_iterate_one's gather at d_pos = double[n][3] into d_out[n] from the window [nalloc][Nmesh][zp]
 *                                 (zp: the slab pitch, or Nmesh + 2): the own planes from plane0 on and behind them the right-hand
 *                                 neighbour's first plane (nalloc = nplanes + 1; one rank: plane0 = 0, nalloc = nplanes = Nmesh).  A
 *                                 position whose Pos / CellSize rounds up to Nmesh is cell 0 with residual 0: rank 0's plane 0.  A
 *                                 particle with a corner outside the window is SHQ_ERR_INVALID and is not written
 *   shq_zeldovich_slab_finalize   the particle loop on d_fld = double[7][n] (rows 4 .. 6 read only with ScaleDepVelocity) into
 *                                 d_pos_out, d_vel, d_disp = double[n][3]; mx = this rank's maxdisp and max |Vel|^2 */
int shq_zeldovich_slab_pitch(int Nmesh);
int shq_zeldovich_slab_fill(shq_context *ctx, int Nmesh, int Seed, int UnitaryAmplitude, int InvertPhase, int y0, int nyl, void *d_spec);
int shq_zeldovich_slab_tables(shq_context *ctx, int Nmesh, double BoxSize, const double *delta, const double *growth);
int shq_zeldovich_slab_xtransfer(shq_context *ctx, int Nmesh, double BoxSize, const void *d_spec, void *d_out, int y0, int nyl, int field);
int shq_zeldovich_slab_transfer(shq_context *ctx, int Nmesh, double BoxSize, const void *d_spec, void *d_out, int y0, int nyl, int field);
int shq_zeldovich_slab_fft_yz(shq_context *ctx, int Nmesh, void *d_planes, int nplanes, const void *d_packed, int nranks);
int shq_zeldovich_slab_gather(shq_context *ctx, int Nmesh, double BoxSize, const void *d_pos, int64_t n, const void *d_mesh, int plane0,
                              int nplanes, int nalloc, void *d_out);
int shq_zeldovich_slab_finalize(shq_context *ctx, int64_t n, const void *d_pos, const void *d_fld, int ScaleDepVelocity, double vel_prefac,
                                double BoxSize, void *d_pos_out, void *d_vel, void *d_disp, double mx[2]);

/* ---- Glass making (glass_evolve, libgenic/glass.cpp:76-360, with petapm_force's deposit and readout, petapm.cpp:1132-1183, and
 * powerspectrum_add_mode, gravpm.cpp:323-376) ----  one rank.  The reversed-gravity PM relaxation loop, resident on the device from
 * the first deposit to the last kick.  Storage types and rounding points are ic_part_data's (allvars.h:8-16): double Pos, float Vel,
 * float Disp, float Mass; the readout rounds the running Disp to float after each of the eight CIC connections. */
typedef struct shq_glass_params {
    int32_t Nmesh;               /* even, 4 .. 2048 */
    int32_t nsteps;              /* >= 0; setup_glass uses 14.  nsteps steps are nsteps + 1 forces */
    double BoxSize;
} shq_glass_params;
typedef struct shq_glass_step {  /* one per step: what the reference prints and what it hands to powerspectrum_save */
    double t_f, t_v, t_x;        /* as glass_evolve advances them (the reference prints them divided by 2 pi) */
    double force_std, vel_std;   /* glass_stats: sqrt(sum Disp^2 / n), sqrt(sum Vel^2 / n) over all three components */
} shq_glass_step;
/* glass_evolve:
 *   pos   : in/out host double [n][3], any finite value.  Positions are never wrapped, on the way in or out: the cell is
 *           floor(Pos / CellSize) taken modulo Nmesh, the residual comes from the unwrapped quotient (the reference's region is built from
 *           the particles' min / max and folded into the mesh periodically)
 *   vel   : in/out host float [n][3];  disp : out host float [n][3], the last force;  mass : in host float [n]
 *   steps : out [nsteps], or NULL
 *   kk, power, nmodes, norm : out [nsteps][Nmesh] (norm: [nsteps]), the raw sums of step s's force before powerspectrum_sum, or all
 *           four NULL.  Every mode is added TWICE, once with the CIC deconvolution weight (measure_power_spectrum) and once with
 *           weight 1 (potential_transfer, glass.cpp:304), into the same bins: that is what the reference saves, not a choice made here.
 *           shq_glass_finish_power turns one step's sums into the saved columns.
 * The force: fixed-point CIC deposit of double(mass), unscaled r2c, every mode but the zero mode times pot_factor * (1.0 / k2) with
 * pot_factor = pow(2 pi / BoxSize, -2) / totmass (PLUS: inverted gravity; no smoothing, no deconvolution), per axis times
 * i * (-diff_kernel(k 2 pi / Nmesh) * (Nmesh / BoxSize)), unscaled c2r, CIC gather into float Disp.  totmass is the double sum of the
 * float masses in particle order, as the reference forms it.
 * The mesh does not depend on particle order or launch shape, so the call is deterministic, and evolve(a + b) equals evolve(a) followed by
 * evolve(b) bit for bit in pos, vel and disp.  A permuted particle order gives the permuted result whenever totmass is the same double
 * (always for equal masses).  The statistics and spectrum sums are accumulated in any order; they do not feed back.
 * SHQ_ERR_INVALID before anything is written for an odd Nmesh or one outside 4 .. 2048, nsteps < 0, a BoxSize that is not finite and > 0,
 * a non-finite position, velocity or mass, a position beyond 2^30 cells from the origin, a total mass that is not > 0, n >= 2^32 (also
 * n < 1), or some but not all of the four spectrum pointers.  Positions outside [0, BoxSize) are valid.
 * The call owns its two meshes and its particle buffers: the resident particle set and tree, the PM mesh and its result, a pending
 * spectrum, the resident Zel'dovich field, the deposit type mask and scale and shq_pm_measure_power's setting survive.  A prestarted PM is
 * joined first, because the transforms share the context's twiddle table with it.  One upload, one download.  Synchronous. */
int shq_glass_evolve(shq_context *ctx, const shq_glass_params *params, int64_t n, double *pos, float *vel, float *disp, const float *mass,
                     shq_glass_step *steps, double *kk, double *power, int64_t *nmodes, double *norm);
/* HIP-event durations (ms) of the last shq_glass_evolve: [0] the upload, [1] all forces (deposit to the third gather), [2] all particle
 * loops, [3] all of it on the device, the download included. */
int shq_glass_phase_ms(shq_context *ctx, double ms[4]);
/* Host only: setup_glass's positions (glass.cpp:49-66) for the whole Ngrid^3 lattice on one rank (ThisTask = 0): the lattice position
 * of index i (x = i / Ngrid^2, y = (i mod Ngrid^2) / Ngrid, z = i mod Ngrid, times BoxSize / Ngrid) plus, per axis in k order,
 * shift + BoxSize / Ngrid * 3 * (u - 0.5), u from one serial mt19937(seed) through uniform_real_distribution<double>(0, 1) read as ONE
 * 32-bit output per draw (raw / 2^32, redrawn if the result is not below 1).  That reading of boost's distribution on a 32-bit engine is
 * the one the Zel'dovich sampler uses; it has not been checked against a boost build.  pos: out [Ngrid^3][3]. */
int shq_glass_setup_positions(int Ngrid, double BoxSize, double shift, int seed, double *pos);
/* Host only: powerspectrum_sum's tail (powerspectrum.cpp:71-87) on one step's raw sums, in place: bins without modes removed, the others
 * Power / Nmodes / Norm * BoxSize_in_MPC^3 and kk / Nmodes * 2 pi / BoxSize_in_MPC, moved to the front.  *nonzero: how many remain. */
int shq_glass_finish_power(int size, double BoxSize_in_MPC, double *kk, double *power, int64_t *nmodes, double norm, int *nonzero);
/* Host only: setup_glass's loop for ONE task's sub-block of the lattice (idgen_init, zeldovich.cpp:46-87): x in [offset[0], offset[0] +
 * size[0]), y in [offset[1], offset[1] + size[1]), every z, in the index order of idgen_create_pos_from_index (x slowest, z fastest),
 * three draws per particle from one serial mt19937(seed).  The reference seeds every task with seed + ThisTask: the caller passes that
 * sum.  offset = {0, 0} and size = {Ngrid, Ngrid} give the bits of shq_glass_setup_positions.  pos: out [size[0] size[1] Ngrid][3]. */
int shq_glass_setup_positions_block(int Ngrid, double BoxSize, double shift, int seed, const int offset[2], const int size[2], double *pos);

/* ---- Glass making on several ranks (shenqi_amd/dist.py, DistGlass): the phases of shq_glass_evolve as entry points of their own, with
 * the caller's exchanges between them.  The reference runs glass_evolve on every task through petapm_force and all-reduces
 * glass_stats' and _prepare's sums (glass.cpp:150-172, 219-258).
 *
 * Every pointer named d_ is DEVICE memory of the caller; nothing is uploaded or downloaded but the tables, the outside-the-window flag
 * and the two statistics sums.  The density's int64 deposit, its (y, z) half spectrum and a force's real mesh live on the rank's x planes,
 * [nalloc][Nmesh][zp] of 8 bytes, zp = shq_glass_slab_pitch(Nmesh) or, for a mesh size without a bespoke transform (pitch 0), Nmesh + 2.
 * The spectrum lives on the rank's y-slab, the mesh rows y0 <= y < y0 + nyl: d_spec = [Nmesh][nyl][zp / 2] complex, x slowest (dense with
 * Nmesh / 2 + 1 without a bespoke transform).  The window of a rank is its own planes from plane0 on and one more plane behind them,
 * nalloc = nplanes + 1: the deposit's ghost plane, or the right-hand neighbour's first plane for the gather; one rank alone has plane0 =
 * 0 and nalloc = nplanes = Nmesh, the periodic mesh.  A particle belongs to the window that holds its CIC base plane
 * (shq_glass_slab_planes): floor(Pos / CellSize) modulo Nmesh with cic.hpp's own arithmetic, so that a position whose quotient rounds up
 * to Nmesh is plane 0 and a negative one folds as the kernels fold it.
 * None of these calls reads or writes the PM's state (mesh, deposit scale, type mask, twiddles, pending spectrum, prestarted PM), the
 * one-rank resident Zel'dovich field or the Zel'dovich slab family's tables: twiddles, tables, flag and sums are the family's own.  They
 * run on the context's stream; tables, deposit, gather and particles return synchronised, the others only launch.
 *
 *   shq_glass_slab_tables    fac[i] = -diff_kernel(k_i 2 pi / Nmesh) * (Nmesh / BoxSize), 1 / sinc^2 per mesh index, the bin of every
 *                            k2 and pot_factor = pow(2 pi / BoxSize, -2) / totmass, in shq_glass_evolve's expressions, kept on the
 *                            device until the next call.  totmass is the sum over ALL ranks
 *   shq_glass_slab_planes    d_planes[p] = the int32 base plane of particle p
 *   shq_glass_slab_deposit   zeroes the window, then the CIC deposit of d_pos = double[n][3] (unwrapped) times double(d_mass[p]) as
 *                            int64 with the scale 2^(61 - exp): exp is frexp's exponent of the total mass of ALL ranks, so that every
 *                            rank count deposits the same integers.  A particle whose base plane is not one of the rank's own is
 *                            SHQ_ERR_INVALID; it deposits nothing, and nothing is ever written outside the window
 *   shq_glass_slab_fft_yz    direction 0: the int64 planes (worth 2^(exp - 61) per unit) to the (y, z) half spectrum; 1: back to real
 *                            space.  d_packed (NULL: in place) is the all-to-all buffer [nranks][nplanes][Nmesh / nranks][zp / 2]
 *                            complex the Y pass writes (0) or reads (1)
 *   shq_glass_slab_xforward  the X forward of the y-slab in place.  With d_sums = double[3 Nmesh + 1] - power[Nmesh], kk[Nmesh],
 *                            nmodes[Nmesh] (uint64), norm - both of the reference's additions are ADDED to it as the tile is stored
 *                            (the caller zeroes it): measure_power_spectrum's with the deconvolution weight and potential_transfer's
 *                            with weight 1 (glass.cpp:304), per mode the operations of the one-rank call.  Only the slab with y = 0
 *                            writes norm.  The spectrum has the same bits with and without sums
 *   shq_glass_slab_xtransfer per mode value *= pot_factor * (1.0 / k2) * f * f (f = 1), the zero mode 0, then (-v.y fa, v.x fa) with
 *                            fa = fac[index along axis], fused into the X inverse and stored OUT OF PLACE into d_out of d_spec's
 *                            shape; d_spec is only read and serves all three axes.  Pad columns z' > Nmesh / 2 are stored as 0
 *   shq_glass_slab_power, shq_glass_slab_transfer   the same sums and the same factor on a dense slab [Nmesh][nyl][Nmesh / 2 + 1],
 *                            between the caller's own X transforms (d_out may be d_spec)
 *   shq_glass_slab_gather    d_disp[3 p + axis] = the float gather of d_mesh (doubles) with the eight roundings in connection order.
 *                            A particle with a corner outside the window is SHQ_ERR_INVALID and is not written
 *   shq_glass_slab_particles one step boundary per particle (the second kick of the step that ends with glass_stats' two terms if
 *                            `ending`, the first kick and the drift of the step that begins if `beginning`); sums = this rank's
 *                            {sum Disp^2, sum Vel^2} (0, 0 without `ending`)
 * SHQ_ERR_STATE from xforward with sums, xtransfer, power and transfer without tables of this Nmesh. */
int shq_glass_slab_pitch(int Nmesh);
int shq_glass_slab_tables(shq_context *ctx, int Nmesh, double BoxSize, double totmass);
int shq_glass_slab_planes(shq_context *ctx, int Nmesh, double BoxSize, const void *d_pos, int64_t n, void *d_planes);
int shq_glass_slab_deposit(shq_context *ctx, int Nmesh, double BoxSize, const void *d_pos, const void *d_mass, int64_t n, int exp, int plane0,
                           int nplanes, int nalloc, void *d_mesh);
int shq_glass_slab_fft_yz(shq_context *ctx, int Nmesh, void *d_planes, int nplanes, int direction, int exp, void *d_packed, int nranks);
int shq_glass_slab_xforward(shq_context *ctx, int Nmesh, void *d_spec, int y0, int nyl, void *d_sums);
int shq_glass_slab_xtransfer(shq_context *ctx, int Nmesh, const void *d_spec, void *d_out, int y0, int nyl, int axis);
int shq_glass_slab_power(shq_context *ctx, int Nmesh, const void *d_spec, int y0, int nyl, void *d_sums);
int shq_glass_slab_transfer(shq_context *ctx, int Nmesh, const void *d_spec, void *d_out, int y0, int nyl, int axis);
int shq_glass_slab_gather(shq_context *ctx, int Nmesh, double BoxSize, const void *d_pos, int64_t n, const void *d_mesh, int plane0, int nplanes,
                          int nalloc, void *d_disp, int axis);
int shq_glass_slab_particles(shq_context *ctx, int64_t n, void *d_pos, void *d_vel, const void *d_disp, int ending, int beginning, double sums[2]);

/* ---- Thermal velocities (add_thermal_speeds with init_rng and init_thermalvel, libgenic/thermal.cpp:44-110, as genic/main.cpp:162-187
 * calls them for warm dark matter and main.cpp:215-228 for neutrino particles) ----  one rank's sub-block of the Ngrid^3 lattice.
 * The reference reseeds one boost::random::ranlux48 at the start of every grid column (x, y) from a table of seeds and takes three
 * uniform draws per particle along z: a Fermi-Dirac speed through the inverse cumulative table, then an isotropic direction.  The
 * columns are independent, so the device runs one engine per lane.
 * Two readings of boost are taken without a boost build to check them against, and everything below rests on them:
 *  - boost::random::ranlux48 is std::ranlux48, discard_block<subtract_with_carry<48, 5, 12>, 389, 11> seeded through the LCG
 *    40014 x mod 2147483563 (boost documents the standard's 10000th value, 249142670248501; the device engine is checked against
 *    libstdc++'s), and uniform_01<double> on it is one output times 2^-48, exact and below 1, so it never redraws;
 *  - boost::math::interpolators::makima is the modified Akima slopes (two ghost secants per side, m[-1] = 2 m[0] - m[1], weights
 *    |m[i+1] - m[i]| + |m[i+1] + m[i]| / 2, slope 0 where both weights vanish; equal to scipy's makima) in a cubic Hermite evaluated as
 *    t = (p - x[i]) / dx,  F = (1 - t)^2 (y[i] (1 + 2 t) + s[i] (p - x[i])) + t^2 (y[i+1] (3 - 2 t) + dx s[i+1] (t - 1)),
 *    in the bin i = the last knot with x[i] <= p, at most 1998.  The order of operations inside F is this library's choice. */
#define SHQ_THERMAL_NKNOTS 2000  /* LENGTH_FERMI_DIRAC_TABLE, thermal.h:10 */
typedef struct shq_thermal_params {
    int32_t Ngrid;               /* >= 2: the lattice of this species (All2.Ngrid or All2.NGridNu) */
    int32_t x0, nx, y0, ny;      /* the rank's sub-block x in [x0, x0 + nx), y in [y0, y0 + ny), every z (idgen_init, zeldovich.cpp:47-65) */
    int32_t pad_;
    double v_amp;                /* thermalvel.m_vamp: NU_V0 or WDM_V0 as the caller forms it */
} shq_thermal_params;
/* Host only: init_rng (thermal.cpp:77-91).  One ranlux48((uint32_t) Seed) gives Ngrid^2 outputs, i outer and j inner, each truncated
 * to 32 bits and stored at table[i + Ngrid * j]: the reference's storage order, which shq_thermal_speeds takes as it is.
 * SHQ_ERR_INVALID for Ngrid outside 1 .. 46340 (Ngrid^2 fits an int) or a NULL table. */
int shq_thermal_seed_table(int Seed, int Ngrid, uint32_t *table);
/* Host only: init_thermalvel's tables (thermal.cpp:44-75) for callers without the reference's struct, SHQ_THERMAL_NKNOTS entries each:
 * max_fd is clipped to 17; vel[i] = min_fd + (max_fd - min_fd) * i / 1999.0; cumprob[i] = the integral of x^2 / (e^x + 1) from min_fd
 * to vel[i] over its last entry (so cumprob[1999] is exactly 1); *total_frac = that last entry over the integral from 0 to 17.
 * The integrals are 8-point Gauss-Legendre sums per knot interval, converged far below 1e-12 relative; the reference's adaptive
 * Gauss-Kronrod rule stops at a looser bound, so its tables differ in the last digits and a reference-side caller passes its own.
 * SHQ_ERR_INVALID for max_fd <= min_fd (after the clip too), a non-finite bound, or a NULL pointer. */
int shq_thermal_tables(double max_fd, double min_fd, double *vel, double *cumprob, double *total_frac);
/* The particle loop of main.cpp:176-184 / 218-226 for one rank:
 *   seedtable : host [Ngrid^2] as shq_thermal_seed_table stores it.  Local particle i is x = i / (ny Ngrid) + x0,
 *               y = (i mod (ny Ngrid)) / Ngrid + y0, z = i mod Ngrid; its id is x Ngrid^2 + y Ngrid + z + 1, its column id / Ngrid =
 *               x Ngrid + y, seeded with seedtable[x Ngrid + y]: draw number y Ngrid + x of the table's stream, the reference's
 *               transposition kept
 *   cumprob, fdvel : host [2000], thermalvel.fermi_dirac_cumprob and fermi_dirac_vel
 *   vel       : in/out host float [n][3], n = nx ny Ngrid, in the rank's particle order
 *   dvel      : out [n][3] or NULL, the double increments exactly as they are added;  speed : out [n] or NULL, each particle's v
 * Per particle three draws in this order: p, v = v_amp * F(p);  phi = (2 * M_PI) * u;  theta = acos(2 * u - 1).  The increments are
 * (v sin theta) cos phi, (v sin theta) sin phi, v cos theta, each added as Vel = (float) ((double) Vel + inc).  No product is fused
 * into an add, so vel_out == float32(float64(vel_in) + dvel) holds bit for bit.  speed follows the evaluation order above with IEEE
 * operations only; the increments carry the device's sin, cos and acos.  The makima slopes are made once per call on the host.
 * SHQ_ERR_INVALID before anything is written for Ngrid < 2 (at Ngrid = 1 the reference indexes past its own table), a sub-block outside
 * the grid, n != nx ny Ngrid or n >= 2^31, a NULL required pointer, a non-finite v_amp or table entry, cumprob[0] != 0,
 * cumprob[1999] != 1, or a cumprob or fdvel that is not strictly increasing.
 * The call owns its buffers: the resident particle set and tree, the PM mesh and its result, a pending spectrum, the resident Zel'dovich
 * field and the deposit settings survive.  One upload, one download.  Synchronous. */
int shq_thermal_speeds(shq_context *ctx, const shq_thermal_params *params, const uint32_t *seedtable, const double *cumprob,
                       const double *fdvel, int64_t n, float *vel, double *dvel, double *speed);
/* HIP-event durations (ms) of the last shq_thermal_speeds: [0] the upload, [1] the kernel, [2] all of it on the device, the download
 * included. */
int shq_thermal_phase_ms(shq_context *ctx, double ms[3]);
/* Test entry for the engine: n engines (n <= 65536), engine t seeded with seeds[t]; raw: out [n][m], the first m outputs of each
 * (1 <= m <= 2^20). */
int shq_thermal_column_draws(shq_context *ctx, int n, const uint32_t *seeds, int m, uint64_t *raw);

/* ---- radiative cooling (cooling_direct, libgadget/sfr_eff.cpp:430-481; DoCooling / GetCoolingTime, cooling.cpp:42-163; the rate network,
 * cooling_rates.cpp:293-305, 499-683, 1101-1214; TableMetalCoolingRate and get_local_UVBG, cooling_uvfluc.cpp:142-214, 321-335) ----------
 * The library evaluates no rate fit and reads no file: the caller hands over the table block init_cooling_rates builds, the interpolated
 * UVBG, the metal table and the Zreion table as data.  One engine (csrc/cooling_math.hpp) serves the device and the host entry.
 * Per particle the outcome is one of four; none ends the call, and a particle whose status is not OK is left exactly as it came: */
#define SHQ_COOL_OK 0        /* computed */
#define SHQ_COOL_DEFERRED 1  /* a rate lookup left the table (T >~ 9.8e8 K or T < 1/e K) where the reference calls the fit: the caller's own
                                cooling_direct takes this particle */
#define SHQ_COOL_BADINPUT 2  /* non-finite temperature, non-positive or non-finite density or energy */
#define SHQ_COOL_NOCONV 3    /* MAXITER (1000) iterations of the fixed point or of the bisection, where the reference ends the run */
#define SHQ_COOL_NSTATUS 4
#define SHQ_COOL_NRECOMBTAB 1000
typedef struct shq_cooling_uvbg { /* struct UVBG, cooling.h:9-19 */
    double J_UV, gJH0, gJHep, gJHe0, epsH0, epsHep, epsHe0, self_shield_dens, zreion;
} shq_cooling_uvbg;
typedef struct shq_cooling_tables {
    const double *rate_tables;    /* [14][1000]: temp_tab as init_cooling_rates lays it out (:989-1024); row 0 (logt) is not read */
    int32_t cooling;              /* enum CoolingType: 0 KWH92, 1 Enzo2Nyx, 2 Sherwood */
    int32_t SelfShieldingOn, HeliumHeatOn, pad_;
    double MinGasTemp, CMBTemperature, HeliumHeatThresh, HeliumHeatAmp, HeliumHeatExp;
    double rho_crit_baryon;       /* cooling_params.rho_crit_baryon */
    double fBar;
    double density_in_phys_cgs, uu_in_cgs, tt_in_s;   /* cooling_units */
    const double *metal;          /* NetCoolingRate [dims[0]][dims[1]][dims[2]] over (redshift, log10 nH, log10 T), or NULL: no metal cooling */
    int32_t metal_dims[3], pad2_; /* each >= 2 */
    double metal_min[3], metal_max[3];
    const double *zreion;         /* UVF.Table [Nside]^3 or NULL */
    int32_t zreion_nside, pad3_;
    double zreion_boxsize;        /* the table's axes run 0 .. BoxSize as init_uvf_table sets them (Step = BoxSize / (Nside - 1)) */
} shq_cooling_tables;
/* The per-run data, copied to the device and kept until replaced.  SHQ_ERR_INVALID for a NULL rate block, a non-finite rate entry, a
 * cooling type outside 0..2, a metal axis shorter than 2 or with max <= min, Nside < 2, or units that are not finite and > 0. */
int shq_cooling_set_tables(shq_context *ctx, const shq_cooling_tables *tables);
/* 1 (default): a wave hands a finished lane the next particle of its workgroup's share of the list, as schedule(guided) does in the
 * reference's loop.  0: one particle per lane.  The results are the same bit for bit. */
int shq_cooling_set_refill(shq_context *ctx, int on);

/* Array-level queries on internal-unit inputs (physical density, as the reference's callers pass it): */
#define SHQ_COOL_UNEW 0       /* DoCooling(redshift, u, rho, dt, uvbg, &ne, Z, MinEgySpec, heiii)                       ne in/out */
#define SHQ_COOL_TCOOL 1      /* GetCoolingTime(redshift, u, rho, uvbg, &ne, Z)                                         ne in/out */
#define SHQ_COOL_NH0 2        /* GetNeutralFraction(u, rho, uvbg, ne)                                                   ne in */
#define SHQ_COOL_HE0 3        /* GetHeliumIonFraction(0, u, rho, uvbg, ne)                                              ne in */
#define SHQ_COOL_HEP 4        /* GetHeliumIonFraction(1, ...) */
#define SHQ_COOL_HEPP 5       /* GetHeliumIonFraction(2, ...) */
#define SHQ_COOL_TEMP 6       /* get_temp(rho cgs, u cgs, 1 - HYDROGEN_MASSFRAC, uvbg, &ne), K                          ne in/out */
#define SHQ_COOL_LAMBDANET 7  /* get_lambdanet of cooling.cpp:42-52, erg / s / g                                        ne in/out */
/*   rho, u, ne : [n];  Z, heiii (bytes), dt : [n], read by UNEW (Z also by TCOOL and LAMBDANET, heiii also by LAMBDANET), may be NULL
 *                otherwise and then count as 0
 *   min_egy_spec : DoCooling's MinEgySpec, internal units;  lmfp_heat : get_long_mean_free_path_heating(z) / (rho_crit_baryon (1+z)^3), added
 *                to the net rate of particles whose heiii byte is 0
 *   out, status : [n]; out is written only where status is SHQ_COOL_OK, as is ne;  steps : [n] or NULL, evaluations of ne_internal
 * shq_cooling_eval needs shq_cooling_set_tables first (SHQ_ERR_STATE) and is synchronous; one upload, one kernel, one download.
 * shq_cooling_eval_host runs the same engine on the CPU over threads and needs neither a context nor a GPU; its results are those of
 * the reference's arithmetic with glibc's libm, evaluation for evaluation. */
int shq_cooling_eval(shq_context *ctx, int what, int64_t n, const double *rho, const double *u, double *ne, const double *Z, const uint8_t *heiii,
                     const double *dt, const shq_cooling_uvbg *uvbg, double redshift, double min_egy_spec, double lmfp_heat, double *out, int32_t *status,
                     int32_t *steps);
int shq_cooling_eval_host(const shq_cooling_tables *tables, int what, int64_t n, const double *rho, const double *u, double *ne, const double *Z,
                          const uint8_t *heiii, const double *dt, const shq_cooling_uvbg *uvbg, double redshift, double min_egy_spec, double lmfp_heat,
                          double *out, int32_t *status, int32_t *steps, int nthreads);
/* cooling_direct (sfr_eff.cpp:430-481) for the active gas of one rank: one call in place of the cooling_direct iterations of
 * cooling_and_starformation's loop (they are independent of the star-forming ones: cooling_direct writes only its own particle).
 * Particles on the effective equation of state are skipped, untouched, and handed back as a list: the input of shq_starformation. */
typedef struct shq_cooling_fields { /* byte offsets in the SPH slot record; all doubles */
    size_t off_ne, off_metallicity, off_sfr, off_delaytime;
} shq_cooling_fields;
#define SHQ_COOL_UVBG_GLOBAL 0   /* every particle sees GlobalUVBG */
#define SHQ_COOL_UVBG_ZREION 1   /* get_local_UVBG_from_global with the Zreion table of shq_cooling_set_tables: eval_periodic at Pos - offset, the
                                    rates zero while zreion < redshift */
#define SHQ_COOL_UVBG_J21 2      /* get_local_UVBG_from_J21: the excursion set's local_J21 and zreion per gas slot */
typedef struct shq_cooling_step {
    double redshift, a3inv, hubble;
    shq_kick_factors kf;                        /* dloga_for_bin is read */
    double lastred_for_bin[SHQ_TIMEBINS + 1];   /* 1 / exp(loga_from_ti(Ti_Current - dti_from_timebin(bin))) - 1: active particles are drifted to Ti_Current */
    shq_cooling_uvbg GlobalUVBG;                /* get_global_UVBG(redshift) */
    int32_t uvbg_mode;                          /* SHQ_COOL_UVBG_* */
    int32_t StarformationOn;
    double HIReionTemp, temp_to_u, MinGasTemp;  /* sfr_params */
    double lmfp_heat;                           /* get_long_mean_free_path_heating(z) / (rho_crit_baryon (1+z)^3), for particles without SHQ_FLAG_HEIII */
    double CurrentParticleOffset[3];
    double PhysDensThresh, OverDensThresh;      /* sfr_params, read when no on_eeqos mask is given */
    /* SHQ_COOL_UVBG_J21 only: */
    const double *local_J21, *zreion;           /* by gas slot */
    double J21_coeffs[6];                       /* struct J21_coeffs of get_J21_coeffs(AlphaUV): gJH0, gJHep, gJHe0, epsH0, epsHep, epsHe0 */
    double ss_greyopac_factor;                  /* pow(greyopac / 2.49e-18, -2./3) of get_self_shield_dens at this redshift */
    double ss_fbar_factor;                      /* pow(fBar / 0.17, -1./3); the device forms 6.73e-3 * A * pow(G12, 2./3) * C in the reference's order */
} shq_cooling_step;
typedef struct shq_cooling_result {
    int64_t n_status[SHQ_COOL_NSTATUS];  /* cooled particles by outcome */
    int64_t n_skipped;                   /* not gas, garbage or Mass <= 0 (sfr_eff.cpp:238) */
    int64_t n_eeqos, n_deferred;         /* entries the two lists would hold */
    int64_t steps;                       /* evaluations of ne_internal, summed */
    double kernel_ms;                    /* HIP-event time of the cooling kernel */
} shq_cooling_result;
/*   parts / sph : Pos, Mass, Type, PI, the flag byte, TimeBinHydro and what shq_sph_state_upload needs; Density, Entropy, DelayTime through PI.
 *                 Uploaded, or skipped under shq_set_inputs_current, as in shq_winds_evolve and shq_heiii_reionization.
 *   list, nlist : the active particles (NULL with nlist == NumPart: all)
 *   on_eeqos    : bytes by particle index, the caller's sfreff_on_eeqos, or NULL: the device then applies its three clauses (:510-517:
 *                 Density a3inv >= PhysDensThresh, Density >= OverDensThresh, DelayTime <= 0).  BHFeedbackUseTcool == 2 adds a fourth
 *                 clause that needs a cooling time per candidate: such a caller MUST pass the mask, which shq_sfr_on_eeqos computes.
 *   eeqos, deferred : out, particle indices in list order: those on the effective equation of state, and the cooled ones that came back
 *                 SHQ_COOL_DEFERRED.  A list shorter than its count is SHQ_ERR_NOMEM after everything else has been written; the result
 *                 holds the counts.
 * Skipped particles and those whose status is not OK are bit-unchanged.  Cooled ones get Ne, Entropy = unew / enttou and Sfr = 0 in the
 * caller's records; the context's Entropy copy is updated alike.  SHQ_ERR_STATE without shq_cooling_set_tables, or for the Zreion mode
 * without a Zreion table.  Synchronous. */
int shq_cooling(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const shq_cooling_fields *fields, const int32_t *list, int64_t nlist,
                const shq_cooling_step *step, const uint8_t *on_eeqos, int32_t *eeqos, int64_t eeqos_capacity, int32_t *deferred, int64_t deferred_capacity,
                shq_cooling_result *result);
/* HIP-event time of the last cooling kernel of the context (shq_cooling_eval or shq_cooling), ms, and the engine steps it summed */
int shq_cooling_last_kernel(shq_context *ctx, double *ms, int64_t *steps);

/* ---- star formation on the effective equation of state ("eeqos"; libgadget/sfr_eff.cpp: sfreff_on_eeqos :502-533, the *_sfreff fractions
 * :536-600, cooling_relaxed :633-668, quicklyastarformation :673-692, starformation :698-767, get_sfr_eeqos :771-809,
 * get_starformation_rate_full :811-830, get_egyeff :833-846, find_star_mass :970-991, the H2 and self-gravity factors :1009-1080) --------
 * One engine (csrc/sfr_math.hpp) on top of the cooling engine serves the device and the host entry.  A particle needs between zero and
 * three GetCoolingTime solves; the statuses are the cooling engine's (SHQ_COOL_*): DEFERRED when a rate lookup left the table in any of
 * the solves (a BH-heated energy above ~1e8 K can do this; the reference's own starformation() takes the particle), BADINPUT, NOCONV.  A
 * particle whose status is not OK is not written and forms no star. */
typedef struct shq_sfr_params { /* what the engine reads of sfr_params */
    int32_t StarformationCriterion;   /* the reference's enum values: 1 density, 3 H2, 5 self-gravity, 13 convergent flow, 21 continuous cutoff */
    int32_t BHFeedbackUseTcool;       /* 0..3 */
    int32_t Generations;              /* >= 1 */
    int32_t BoostSFDenseGas;
    int32_t winds_subgrid;            /* WindOn && winds_are_subgrid() */
    int32_t pad_;
    double PhysDensThresh, OverDensThresh, EgySpecSN, EgySpecCold, FactorSN, FactorEVP, MaxSfrTimescale, tau_fmol_unit;
    double QuickLymanAlphaProbability, QuickLymanAlphaTempThresh, avg_baryon_mass, temp_to_u, UnitSfr_in_solar_per_year;
    double BoostSFOverDenseFactor, GravInternal;
} shq_sfr_params;
typedef struct shq_sfr_arrays { /* [n] each */
    const double *Density, *Entropy, *Ne, *Metallicity, *Mass;
    const double *Hsml, *DivVel, *CurlVel;   /* read by the H2 / self-gravity factors; NULL counts as 0 */
    const double *GradRho;                   /* |GradRho|; NULL unless StarformationCriterion has the H2 bits (then SHQ_ERR_INVALID, the reference's endrun) */
    const double *dloga;                     /* get_dloga_for_bin(TimeBinHydro, Ti_drift) */
    const double *DelayTime;                 /* NULL: 0 */
    const uint8_t *timebin;                  /* TimeBinHydro */
    const uint8_t *flags;                    /* the particle flag byte: bit 3 BHHeated, bits 4-7 Generation */
    const uint64_t *ID;
} shq_sfr_arrays;
typedef struct shq_sfr_eval_step {
    double redshift, a3inv, hubble;
    shq_cooling_uvbg GlobalUVBG;   /* read by get_egyeff: the fourth clause of sfreff_on_eeqos, and the EGYEFF query */
    shq_cooling_uvbg LocalUVBG;    /* get_local_UVBG's result, read by get_sfr_eeqos, cooling_relaxed and the fractions */
    const double *rnd_table;       /* RandTable::Table: get_random_number(id) = rnd_table[id % rnd_size] */
    int64_t rnd_size;
} shq_sfr_eval_step;
/* what to evaluate */
#define SHQ_SFR_STARFORM 0    /* starformation() for every particle given; with QuickLymanAlphaProbability > 0 quicklyastarformation and, for a
                                 hit, the conversion of the parent with sm = Mass: no eeqos physics runs */
#define SHQ_SFR_EGYEFF 1      /* get_egyeff(redshift, Density, GlobalUVBG): Density is the argument as it stands; its tsfr and egyhot in their rows */
#define SHQ_SFR_NH0 2         /* get_neutral_fraction_sfreff */
#define SHQ_SFR_HE0 3         /* get_helium_neutral_fraction_sfreff(0, ...) */
#define SHQ_SFR_HEP 4         /* ... (1, ...) */
#define SHQ_SFR_HEPP 5        /* ... (2, ...) */
#define SHQ_SFR_ON_EEQOS 6    /* sfreff_on_eeqos, all four clauses: bit 0 of the branch byte */
#define SHQ_SFR_NWHAT 7
/* rows of out [SHQ_SFR_NOUT][n] */
#define SHQ_SFR_O_TRELAX 0        /* sfr_eeqos_data: trelax, tsfr, egyhot, egycold, cloudfrac, ne; their initial values when not on the eeqos */
#define SHQ_SFR_O_TSFR 1
#define SHQ_SFR_O_EGYHOT 2
#define SHQ_SFR_O_EGYCOLD 3
#define SHQ_SFR_O_CLOUDFRAC 4
#define SHQ_SFR_O_NE_EEQOS 5
#define SHQ_SFR_O_SMR 6           /* get_starformation_rate_full */
#define SHQ_SFR_O_SM 7            /* smr * dtime: StellarMass of the subgrid winds */
#define SHQ_SFR_O_DM 8            /* sum_sm's addend */
#define SHQ_SFR_O_SFR 9           /* SPHP.Sfr: localsfr's addend */
#define SHQ_SFR_O_NE 10           /* the record's new Ne, Metallicity, Entropy */
#define SHQ_SFR_O_METALLICITY 11
#define SHQ_SFR_O_ENTROPY 12
#define SHQ_SFR_O_MASS_OF_STAR 13
#define SHQ_SFR_O_PROB 14
#define SHQ_SFR_O_QUERY 15        /* the value of EGYEFF / NH0 / HE0 / HEP / HEPP */
#define SHQ_SFR_O_EGYEFF4 16      /* get_egyeff of the fourth clause (BHFeedbackUseTcool == 2), 0 when it did not run */
#define SHQ_SFR_O_TCOOL_RELAX 17  /* cooling_relaxed's cooling time, 0 when it did not run */
#define SHQ_SFR_O_EGYEFF 18       /* cooling_relaxed's egyeff and egycurrent, 0 when it did not run */
#define SHQ_SFR_O_EGYCURRENT 19
#define SHQ_SFR_O_TRELAX_USED 20  /* the relaxation time after the tcool < trelax test */
#define SHQ_SFR_O_DTIME 21        /* dloga / hubble: sum_dtime's addend */
#define SHQ_SFR_O_FACTOREVP 22    /* get_sfr_eeqos' factorEVP, cooling_relaxed's entropy_to_u, starformation's 1 - exp(-p); 0 when not computed */
#define SHQ_SFR_O_DENSITYFAC 23
#define SHQ_SFR_O_FRAC 24
#define SHQ_SFR_NOUT 25
/* the decision byte */
#define SHQ_SFR_NONE 0
#define SHQ_SFR_CONVERT 1     /* the parent becomes the star */
#define SHQ_SFR_SPLIT 2       /* Mass >= 1.1 mass_of_star: slots_split_particle(parent, mass_of_star) */
/* the branch byte: which way the particle went */
#define SHQ_SFR_B_ON_EEQOS 1u   /* sfreff_on_eeqos */
#define SHQ_SFR_B_CLAUSE4 2u    /* its fourth clause was evaluated */
#define SHQ_SFR_B_TCOOL 4u      /* cooling_relaxed computed a cooling time (egycurrent > egyeff inside the BHFeedbackUseTcool clause) */
#define SHQ_SFR_B_TCOOL_WON 8u  /* tcool < trelax && tcool > 0 */
#define SHQ_SFR_B_STAR 16u      /* the draw was below prob */
#define SHQ_SFR_B_RELAXED 32u   /* dloga > 0 && TimeBinHydro: cooling_relaxed ran */
/*   out         : [SHQ_SFR_NOUT][n]; column k is written only where status[k] is SHQ_COOL_OK, as are the three bytes of k
 *   flags_out   : the flag byte with BHHeated cleared where cooling_relaxed clears it;  decision : SHQ_SFR_NONE / _CONVERT / _SPLIT
 *   steps       : [n] or NULL, evaluations of ne_internal over all solves of the particle
 * shq_sfr_eval needs shq_cooling_set_tables first (SHQ_ERR_STATE) and is synchronous: one upload, one kernel, one download.  The random
 * table is staged in the context's buffer that the winds and black-hole entries use.  shq_sfr_eval_host runs the same engine on the CPU
 * over threads and needs neither a context nor a GPU; its results are those of the reference's arithmetic with glibc's libm.
 * SHQ_ERR_INVALID for Generations < 1, an empty random table, or a NULL GradRho with the H2 bits set. */
int shq_sfr_eval(shq_context *ctx, const shq_sfr_params *par, int what, int64_t n, const shq_sfr_arrays *in, const shq_sfr_eval_step *step, double *out,
                 uint8_t *flags_out, uint8_t *decision, uint8_t *branch, int32_t *status, int32_t *steps);
int shq_sfr_eval_host(const shq_cooling_tables *tables, const shq_sfr_params *par, int what, int64_t n, const shq_sfr_arrays *in, const shq_sfr_eval_step *step,
                      double *out, uint8_t *flags_out, uint8_t *decision, uint8_t *branch, int32_t *status, int32_t *steps, int nthreads);
/* 1 (default): a finished lane takes the next particle of its workgroup's share, as in shq_cooling_set_refill.  0: one particle per lane.
 * Each particle is written by exactly one lane: the results are the same bit for bit. */
int shq_sfr_set_refill(shq_context *ctx, int on);
/* HIP-event time of the context's last star-formation kernel, ms, and the engine steps it summed */
int shq_sfr_last_kernel(shq_context *ctx, double *ms, int64_t *steps);

/* The star-forming branch of cooling_and_starformation (sfr_eff.cpp:252-276) for one rank: one call in place of the reference's
 * starformation() iterations over the particles on the effective equation of state.  The call chain of a step is
 *   shq_winds_evolve -> shq_sfr_on_eeqos (BHFeedbackUseTcool == 2 only) -> shq_cooling -> shq_starformation ->
 *   shq_slots_split_particles -> shq_make_particle_stars;  add_new_particle_to_active / copy_gravaccel_new_particle stay with the caller. */
typedef struct shq_sfr_fields { /* byte offsets in the SPH slot record; all doubles */
    size_t off_ne, off_metallicity, off_sfr;
    size_t off_delaytime;   /* must equal the SPH view's off_delaytime (SHQ_ERR_INVALID otherwise): DelayTime is staged with the view's fields */
} shq_sfr_fields;
typedef struct shq_sfr_result {
    int64_t n_status[SHQ_COOL_NSTATUS];  /* list entries by outcome */
    int64_t n_skipped;                   /* not gas, garbage or Mass <= 0 */
    int64_t n_newstars, n_split;         /* entries NewParents would hold, and how many of them split */
    int64_t n_maybewind, n_deferred;     /* entries the other two lists would hold */
    int64_t sum_sf_part;                 /* particles that formed stars or were considered for it: the OK ones (quick Lyman-alpha: the hits) */
    double localsfr, sum_sm, sum_dtime;  /* the reference's three reductions.  The per-particle addends (Sfr, dM, dtime) are formed on the
                                            device and added here on the host, left to right in list order, so the sums are reproducible
                                            bit for bit; the reference's OpenMP reduction has no defined order. */
    int64_t steps;                       /* evaluations of ne_internal, summed */
    double kernel_ms;                    /* HIP-event time of the kernel */
} shq_sfr_result;
/* sfreff_on_eeqos (:502-533) for the particles of a list, all four clauses on the device; the fourth (BHFeedbackUseTcool == 2) is one
 * get_egyeff solve per particle that passed the first three.  on_eeqos: [numpart] bytes, written for every particle (0 off the list, for
 * non-gas, garbage and Mass <= 0, and where the solve did not end OK): the form shq_cooling's on_eeqos argument takes.  Views, staging
 * and shq_set_inputs_current as in shq_cooling; step->StarformationOn (0: every byte is 0, as :506 returns), GlobalUVBG and a3inv are
 * read.  SHQ_ERR_STATE without shq_cooling_set_tables. */
int shq_sfr_on_eeqos(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const shq_sfr_params *par, const int32_t *list, int64_t nlist,
                     const shq_cooling_step *step, uint8_t *on_eeqos);
/*   parts / sph, fields : as in shq_cooling (uploaded, or taken as they are under shq_set_inputs_current)
 *   ids          : particle IDs by particle index;  GradRho : |GradRho| by gas slot, NULL unless the H2 bits are set
 *   list, nlist  : the particles on the effective equation of state, i.e. the eeqos list shq_cooling returned.  With
 *                  QuickLymanAlphaProbability > 0 instead the active list: the call classifies it itself with quicklyastarformation
 *                  (:673-692), every hit is a conversion of the parent with sm = Mass, no eeqos physics runs and no record is written.
 *   step         : the shq_cooling_step of the step: redshift, a3inv, hubble, dloga_for_bin, the UVBG mode and its data
 *   rnd_table    : RandTable::Table, staged in the context's buffer of the winds and black-hole entries
 * Out, all in list order; a list shorter than its count is SHQ_ERR_NOMEM after everything else has been written, the result holds the counts:
 *   NewParents, mass_of_star, split [newstar_capacity] : the particles that form a star; split[k] != 0: slots_split_particle(parent, mass_of_star).
 *                  The split ones with their masses are the input of shq_slots_split_particles, all of them (children in place of the
 *                  split parents) that of shq_make_particle_stars.
 *   MaybeWind, sm [maybewind_capacity] : only with par->winds_subgrid, the particles that formed no star: shq_winds_subgrid's list and
 *                  StellarMasses.
 *   deferred [deferred_capacity] : SHQ_COOL_DEFERRED particles, bit-unchanged, for the reference's own starformation().
 * OK particles get Sfr, Ne, Metallicity, Entropy and the cleared BHHeated bit in the caller's records; the context's Entropy copy is
 * updated alike.  Everything else is bit-unchanged.  Synchronous. */
int shq_starformation(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const shq_sfr_fields *fields, const uint64_t *ids, const double *GradRho,
                      const shq_sfr_params *par, const int32_t *list, int64_t nlist, const shq_cooling_step *step, const double *rnd_table, int64_t rnd_size,
                      int32_t *NewParents, double *mass_of_star, uint8_t *split, int64_t newstar_capacity, int32_t *MaybeWind, double *sm, int64_t maybewind_capacity,
                      int32_t *deferred, int64_t deferred_capacity, shq_sfr_result *result);

/* ---- Snapshot blocks: selection, typed columns, readout (libgadget/petaio.cpp, fofpetaio.cpp; csrc/snapshot.hip) ------------------------
 * The three per-particle loops of a snapshot on device-resident records, in the conventions of shq_exchange_*: particle_data[] and the
 * slot arrays are opaque bytes behind device pointers, fields are byte offsets, counts come back through host int64_t.
 *   petaio_build_selection (petaio.cpp:86-128), fof_select_func (fofpetaio.cpp:33-36)        shq_io_select
 *   petaio_build_buffer (:550-575) with the getters (:673-894, :1012-1023)                   shq_io_gather
 *   GTNeutralHydrogenFraction ... GTHeliumIIIFraction (:817-849)                             shq_io_ion_fractions
 *   petaio_readout_buffer (:536-545) with the setters (:684-893)                             shq_io_scatter
 * bigfile I/O, the header, the neutrino blocks and the FOF group blocks stay with the caller. */
#define SHQ_IO_SELECT_ALL 0   /* the reference's NULL select function */
#define SHQ_IO_SELECT_FOF 1   /* fof_select_func: GrNr >= 0 && !Swallowed */
#define SHQ_IO_ORDER_INDEX 0  /* every type in index order (the serial second loop of petaio_build_selection) */
#define SHQ_IO_ORDER_GRNR 1   /* every type in order of GrNr, ties in index order: what fof_distribute_particles' local sort
                                 (fofpetaio.cpp:365-374) leaves for the selection that follows it; the reference's sort is unstable among equal
                                 GrNr, this one is stable, as in shq_slots_gc_sorted */
typedef struct shq_io_layout {
    size_t part_elsize, off_flags, off_type, off_pi;   /* as shq_exchange_layout: bit 0 of the flag byte IsGarbage, bit 1 Swallowed */
    size_t off_grnr;                                   /* int64 GrNr; read by SHQ_IO_SELECT_FOF and SHQ_IO_ORDER_GRNR only */
    size_t slot_elsize[6];                             /* 0: the type has no slots */
} shq_io_layout;
/* petaio_build_selection: d_selection (int32[numpart], device) receives the indices of the particles that are not garbage and pass the
 * predicate, grouped by type: type t at offset[t] = sum of count[< t].  Entries behind the last selected one are unspecified.  A selected
 * particle with Type > 5 is SHQ_ERR_INVALID.  Synchronous (count and offset are host arrays). */
int shq_io_select(shq_context *ctx, const shq_io_layout *layout, const void *d_parts, int64_t numpart, int predicate, int order, int32_t *d_selection,
                  int64_t count[6], int64_t offset[6]);

/* A block: where one column of a snapshot comes from (getter) or goes to (setter).  `field_type` is the type of the member in the record,
 * `col_type` the type of the column in the file ("f8" "f4" "u8" "u4" "i4" "u1" are SHQ_IO_F64 _F32 _U64 _U32 _I32 _U8). */
#define SHQ_IO_SRC_BASE 0   /* particle_data */
#define SHQ_IO_SRC_SLOT 1   /* the slot of the call's ptype, through PI */
#define SHQ_IO_F64 0
#define SHQ_IO_F32 1
#define SHQ_IO_I64 2
#define SHQ_IO_U64 3
#define SHQ_IO_I32 4
#define SHQ_IO_U32 5
#define SHQ_IO_I8 6
#define SHQ_IO_U8 7
#define SHQ_IO_BITS 8       /* bit_width bits from bit_shift of the byte at offset (HeIIIionized, Swallowed, Generation); field type only */
#define SHQ_IO_COPY 0            /* SIMPLE_GETTER(_PI) / SIMPLE_SETTER(_PI): out[k] = (col) field[k], field[k] = (field) in[k], C conversions;
                                    the bit-field form writes only its bits */
#define SHQ_IO_POSITION 1        /* GTPosition / GTBlackholeMinPotPos: out = x - CurrentParticleOffset[d]; while(out > BoxSize) out -= BoxSize;
                                    while(out <= 0) out += BoxSize; each loop at most 64 rounds.  A non-finite value or a loop that does not end
                                    is SHQ_ERR_INVALID (the reference would spin).  As a setter a plain copy (STPosition removes no offset). */
#define SHQ_IO_SCALE 2           /* GTVelocity: out = (col) (fac * field[d]); STVelocity: field[d] = in[d] * fac */
#define SHQ_IO_INTERNAL_ENERGY 3 /* GTInternalEnergy: (float) (Entropy / GAMMA_MINUS1 * pow(Density * a3inv, GAMMA_MINUS1)); STInternalEnergy:
                                    Entropy = GAMMA_MINUS1 * u / pow(Density * a3inv, GAMMA_MINUS1).  offset = Entropy, offset2 = Density */
#define SHQ_IO_MAXBLOCKS 48      /* blocks per kernel launch; longer arrays are served in several launches */
typedef struct shq_io_block {
    int32_t source, kind, field_type, col_type;
    int32_t items;                  /* consecutive members of field_type from offset */
    int32_t bit_shift, bit_width;   /* SHQ_IO_BITS */
    int32_t pad_;
    uint64_t offset, offset2;
} shq_io_block;
typedef struct shq_io_conv {
    double fac;                       /* SCALE: getter 1 / atime under UsePeculiarVelocity else 1; setter atime else 1 */
    double atime;                     /* INTERNAL_ENERGY: a3inv = 1 / (atime * atime * atime) */
    double BoxSize;                   /* POSITION */
    double CurrentParticleOffset[3];
} shq_io_conv;
/* petaio_build_buffer for all blocks of one particle type in one pass: column b (d_out[b], device) is dense [n][items_b] of its col_type,
 * row k belongs to particle d_selection[k].  A record is read from HBM once per call: a tile of selected records is staged in LDS, then
 * one lane per record picks the fields; slot records reached through PI go through the same code.  Checked before the dependent read,
 * each SHQ_ERR_INVALID with the outputs unspecified: a selection index outside [0, numpart); a selected particle whose Type != ptype
 * ("Selection %d has type ...", :569-571); a PI outside [0, slot_size[ptype]) when a block reads the slot.  Records and slot arrays must be
 * 8-byte aligned with sizes that are multiples of 8 and at most 480 bytes.  Synchronous (the status comes from the device). */
int shq_io_gather(shq_context *ctx, const shq_io_layout *layout, const void *d_parts, int64_t numpart, const void *const d_slots[6], const int64_t slot_size[6],
                  int ptype, const int32_t *d_selection, int64_t n, const shq_io_block *blocks, int nblocks, const shq_io_conv *conv, void *const d_out[]);
/* petaio_readout_buffer: the k-th particle of Type == ptype in index order (garbage included: the reference has no garbage test there) takes
 * row k of every column d_in[b] (device, dense [n][items_b] of col_type).  Blocks are applied in array order per particle: STInternalEnergy
 * reads the Density an earlier block of the call may have written.  Each particle is written by one lane.  n != the number of particles
 * of the type, or a PI outside the slot array when a block writes the slot, is SHQ_ERR_INVALID before anything is written. */
int shq_io_scatter(shq_context *ctx, const shq_io_layout *layout, void *d_parts, int64_t numpart, void *const d_slots[6], const int64_t slot_size[6], int ptype,
                   int64_t n, const shq_io_block *blocks, int nblocks, const shq_io_conv *conv, const void *const d_in[]);

/* The four ion-fraction columns: get_neutral_fraction_sfreff and get_helium_neutral_fraction_sfreff(0 / 1 / 2) (sfr_eff.cpp:536-600) for the
 * gas particles of a list, by the engine of shq_sfr_eval (SHQ_SFR_NH0 ... SHQ_SFR_HEPP) with the per-particle local UVBG of shq_cooling
 * (step->uvbg_mode) and dloga_for_bin[TimeBinHydro].  Views, staging and shq_set_inputs_current as in shq_starformation.
 *   list, n      : particle indices (host), e.g. the gas part of a selection; NULL: all particles
 *   which_mask   : bit q set: out[q] (host, [n] floats) receives (float) of query q: 0 NH0, 1 HeI, 2 HeII, 3 HeIII
 *   status [n]   : the first outcome other than SHQ_COOL_OK among the particle's queries, else SHQ_COOL_OK
 *   listed       : the list positions whose status is not SHQ_COOL_OK, in order: their rows hold a quiet NaN and are the caller's to fill with
 *                  the reference's own function (the contract of the deferred lists).  More than listed_capacity: SHQ_ERR_NOMEM after
 *                  everything else has been written.
 * SHQ_ERR_STATE without shq_cooling_set_tables. */
typedef struct shq_io_ion_result {
    int64_t n_status[SHQ_COOL_NSTATUS];
    int64_t n_listed;
    int64_t steps;
    double kernel_ms;
} shq_io_ion_result;
int shq_io_ion_fractions(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const shq_sfr_fields *fields, const shq_sfr_params *par,
                         const shq_cooling_step *step, const int32_t *list, int64_t n, int which_mask, float *const out[4], int32_t *status, int32_t *listed,
                         int64_t listed_capacity, shq_io_ion_result *result);

/* ---- Light-cone crossings: replicas, sampling, ordered rows (libgadget/lightcone.cpp; csrc/lightcone.hip) --------------------------------
 * lightcone_compute (run.cpp:687) on device-resident records, in the conventions of shq_io_* / shq_exchange_*.
 *   lightcone_get_horizon (:101-115)                     shq_lightcone_horizon    host
 *   lightcone_init, the statics' start (:95)             shq_lightcone_init       host
 *   lightcone_set_time, update_replicas (:118-200)       shq_lightcone_set_time   host
 *   the loop over lightcone_cross (:159-168, :203-250)   shq_lightcone_compute    device
 * The three host functions replay the reference statement by statement (same expression order, same int truncation of the bin) and
 * need no GPU.  The table is the caller's (the reference integrates it with boost's Gauss-Kronrod rule); the output file too.
 *
 * Lines :219-220 of the reference read the velocity of record i, the REPLICA index, and add no replica shift to the new position, so
 * |pnew| stays below about the box diagonal and nothing crosses a horizon beyond it.  Two modes:
 *   SHQ_LIGHTCONE_CONSISTENT  velocity of particle p, the replica shift on both ends (what the file's comments describe)
 *   SHQ_LIGHTCONE_AS_WRITTEN  :219-220 literally: the same set of rows as the reference's call; needs numpart >= Nreplica */
#define SHQ_LIGHTCONE_MAXREPLICA 1000
#define SHQ_LIGHTCONE_CONSISTENT 0
#define SHQ_LIGHTCONE_AS_WRITTEN 1
typedef struct shq_lightcone_params {
    double zmin, zmax, ReferenceRedshift;   /* reference: 0.1, 80, 2.0 */
    int32_t BoxBoost, pad_;                 /* reference: 20 */
} shq_lightcone_params;
typedef struct shq_lightcone_table {
    const double *tab_loga, *tab_Dc;        /* host, nentry each: tab_loga[i] = -dloga * (nentry - i - 1), comoving distance to a = exp(tab_loga[i]) */
    int32_t nentry, pad_;
    double dloga;
} shq_lightcone_table;
typedef struct shq_lightcone_state {        /* the reference's file statics */
    double HorizonDistance, HorizonDistance2, HorizonDistancePrev, HorizonDistance2Prev, HorizonDistanceRef, SampleFraction;
    int32_t Nreplica, pad_;
    double Reps[SHQ_LIGHTCONE_MAXREPLICA][3];
} shq_lightcone_state;
typedef struct shq_lightcone_layout {
    size_t part_elsize, off_type, off_pos, off_vel, off_id;   /* double Pos[3], double Vel[3] (MyFloat as shq_part_view has it), uint64 ID, the Type byte as in shq_io_layout */
} shq_lightcone_layout;

/* Linear interpolation of the table in log a; the bin truncates toward zero, the result clamps at both ends.  a <= 0, a NULL or a table
 * of fewer than 2 entries or dloga <= 0: SHQ_ERR_INVALID. */
int shq_lightcone_horizon(const shq_lightcone_table *t, double a, double *Dc);
/* All of the state zero but HorizonDistanceRef = horizon(1 / (1 + ReferenceRedshift)). */
int shq_lightcone_init(const shq_lightcone_table *t, const shq_lightcone_params *p, shq_lightcone_state *s);
/* Inside zmin < z < zmax: the horizons move to Prev, the new horizon, the replica list (rx-major, then ry, then rz; the 1001st is
 * SHQ_ERR_INVALID, "too many replica", the state then holding the first 1000), SampleFraction.  Outside the
 * window only SampleFraction = 0.  BoxBoost outside 1 .. 1290 (BoxBoost^3 fits an int) is SHQ_ERR_INVALID. */
int shq_lightcone_set_time(const shq_lightcone_table *t, const shq_lightcone_params *p, double a, double BoxSize, shq_lightcone_state *s);
/* The crossings of every Type-1 particle (garbage or not: the reference has no garbage test) with every replica of the state.
 *   d_parts    : device, numpart records of layout->part_elsize bytes, 8-byte aligned; numpart in [0, 2^31 - 200)
 *   ddrift, CurrentParticleOffset : as the reference's arguments; finite
 *   rnd_table  : RandTable::Table on the host (rnd_size > 0 entries), staged in the context's buffer of the winds and star-formation
 *                entries; the draw of (p, i) is rnd_table[(ID + i) % rnd_size], the sum wrapping in uint64
 *   d_rows     : device, [capacity][4] doubles: x, y, z of the interpolated crossing, SampleFraction
 *   d_index, d_replica : device, int32[capacity], either may be NULL: the particle index and the replica index of each row
 *   *nrows     : always the number of crossings found
 * Rows are ordered by particle index, then by replica index: the reference's loop on one thread.  The bytes are reproducible.
 * *nrows > capacity: nothing is written, SHQ_ERR_NOMEM; repeat the call with room.  SampleFraction <= 0 or Nreplica == 0: zero rows,
 * no launch.  SHQ_ERR_INVALID with nothing written for a NULL argument, a part_elsize that is no multiple of 8 or outside 8 .. 480, a
 * member outside the record or misaligned, numpart out of range, rnd_size <= 0, a non-finite ddrift, offset or horizon, Nreplica outside
 * 0 .. SHQ_LIGHTCONE_MAXREPLICA, an unknown mode, AS_WRITTEN with numpart < Nreplica.  All f64, no contraction, IEEE sqrt and divide.
 * Synchronous. */
int shq_lightcone_compute(shq_context *ctx, const shq_lightcone_layout *layout, const void *d_parts, int64_t numpart, const shq_lightcone_state *s, int mode,
                          double ddrift, const double CurrentParticleOffset[3], const double *rnd_table, int64_t rnd_size, double *d_rows, int32_t *d_index,
                          int32_t *d_replica, int64_t capacity, int64_t *nrows);
/* Device times of the last shq_lightcone_compute that launched, in ms: pass A (counts), the scan, pass B (rows; 0 when nothing crossed). */
int shq_lightcone_phase_ms(shq_context *ctx, double ms[3]);

/* ---- Run start-up: init()'s loops, the first Hsml, the initial entropy (libgadget/init.cpp, density2.cpp:154-204; csrc/startup.hip) ----
 * What the reference does between petaio_read_snapshot and the first step:
 *   get_mean_separation (init.cpp:390-397)                        shq_startup_mean_separation     host
 *   u_init of setup_smoothinglengths (:467-498)                   shq_startup_u_init              host
 *   check_omega's verdict (:223-236)                              shq_startup_omega               host
 *   check_omega's / check_positions' / check_smoothing_length's / init()'s particle loops (:203-214, :313-335, :342-359, :119-188)
 *                                                                 shq_startup_particles           device records
 *   check_density_entropy (:363-388)                              shq_startup_check_density_entropy   device slots
 *   set_init_hsml (density2.cpp:164-203)                          shq_set_init_hsml               resident particles + current tree
 *   Entropy from u_init (init.cpp:422-423, :518)                  shq_init_entropy                resident gas
 *   setup_smoothinglengths + setup_density_indep_entropy (:402-521)   shq_setup_smoothinglengths  host views, one upload
 * The reference ends the run on the conditions these loops find; here they are reported and the caller decides. */

/* Host functions.  mean_separation: MeanSeparation[t] = BoxSize / pow(NTotalInit[t], 1.0 / 3) where NTotalInit[t] > 0, other entries are
 * left as they are.  u_init: InitGasTemp < 0 becomes CMBTemperature / atime (*InitGasTemp_used, may be NULL, receives the temperature
 * used); u = 1 / GAMMA_MINUS1 * (BOLTZMANN / PROTONMASS) * T / uu_in_cgs / molecular_weight, the weight of full ionisation above 1e4 K
 * and of neutral gas otherwise, floored at MinEgySpec.  omega: omegas[t] = mass_type[t] / (BoxSize^3 RhoCrit), *omega = mass_total /
 * (BoxSize^3 RhoCrit) + (MassiveNuLinRespOn ? OmegaNu : 0), *bad = |omega - Omega0| > 1.0e-3.  meanbar: check_density_entropy's mean
 * baryon density, OmegaBaryon 3 (HUBBLE HubbleParam)^2 / (8 pi GRAVITY) in the reference's order. */
int shq_startup_mean_separation(double MeanSeparation[6], double BoxSize, const int64_t NTotalInit[6]);
int shq_startup_u_init(double InitGasTemp, double CMBTemperature, double atime, double uu_in_cgs, double MinEgySpec, double *u_init, double *InitGasTemp_used);
int shq_startup_omega(const double mass_type[6], double mass_total, double BoxSize, double RhoCrit, double OmegaNu, int MassiveNuLinRespOn, double Omega0,
                      double omegas[6], double *omega, int *bad);
int shq_startup_meanbar(double OmegaBaryon, double HubbleParam, double *meanbar);

/* Where the members the loops touch lie: byte offsets into the particle record, the gas slot and the black-hole slot (element sizes
 * multiples of 8, at most 480; every member inside its record and aligned to its own size).  sph_off_local_j21 / sph_off_zreion may be
 * SHQ_NOFIELD (a build without EXCUR_REION); every other member is required.  The particle record is at most 240 bytes (a tile of 256
 * records is staged in LDS).  Members: double Pos[3], float Mass, the flag byte
 * (Generation in its upper four bits), the Type byte, int32 PI, double Hsml, int64 Ti_drift; gas slot doubles Density, EgyWtDensity,
 * Entropy, DtEntropy, MaxSignalVel, HydroAccel[3], DhsmlEgyDensityFactor, DivVel, CurlVel, Sfr, Ne, DelayTime, Metallicity,
 * float Metals[sph_nmetals], double local_J21, zreion; black-hole slot doubles Mass, DFAccel[3], DragAccel[3]. */
typedef struct shq_startup_layout {
    size_t part_elsize, off_pos, off_mass, off_flags, off_type, off_pi, off_hsml, off_ti_drift;
    size_t sph_elsize, sph_off_density, sph_off_egywtdensity, sph_off_entropy, sph_off_dtentropy, sph_off_maxsignalvel, sph_off_hydroaccel,
        sph_off_dhsmlegydensityfactor, sph_off_divvel, sph_off_curlvel, sph_off_sfr, sph_off_ne, sph_off_delaytime, sph_off_metallicity, sph_off_metals,
        sph_nmetals, sph_off_local_j21, sph_off_zreion;
    size_t bh_elsize, bh_off_mass, bh_off_dfaccel, bh_off_dragaccel;
} shq_startup_layout;

#define SHQ_STARTUP_OMEGA 1       /* check_omega's loop: Mass == 0 recovered from MassTable and Generation, badmass, the mass sums */
#define SHQ_STARTUP_POSITIONS 2   /* check_positions: coordinates outside [0, BoxSize] or not finite; particles at the origin */
#define SHQ_STARTUP_HSML 4        /* check_smoothing_length: Hsml > BoxSize || Hsml <= 0 of types 0 and 5 becomes MeanSeparation[Type] */
#define SHQ_STARTUP_INIT 8        /* init()'s field-initialisation loop */
typedef struct shq_startup_params {
    double BoxSize;
    double MassTable[6];
    double MeanSeparation[6];
    int64_t Ti_Current;
    int32_t generations;          /* get_generations() */
    int32_t RestartSnapNum;       /* -1: initial conditions */
    int32_t init_reion;           /* the condition of init.cpp:183: ExcursionSetReionOn && TimeSnapshot < 1 / (1 + ExcursionSetZStart) */
    int32_t pad_;
} shq_startup_params;
typedef struct shq_startup_report {
    double mass_type[6], mass_total;   /* OMEGA: per rank; the caller all-reduces them */
    int64_t badmass;                   /* OMEGA: masses recovered */
    int64_t noutside, first_outside;   /* POSITIONS: particles with a coordinate < 0, > BoxSize or not finite; the lowest such index or -1 */
    int64_t numzero, lastzero;         /* POSITIONS: particles with every coordinate < 1e-35; the highest such index or -1 */
    int64_t numprob, lastprob;         /* HSML: smoothing lengths replaced; the highest such index or -1 */
    int64_t nbad_delaytime, first_bad_delaytime; /* INIT: gas with a non-finite DelayTime; the lowest such index or -1 */
} shq_startup_report;
/* One pass over the records for every loop in `which` (in the reference's order per record: OMEGA, POSITIONS, HSML, INIT).  d_parts:
 * numpart records, d_sph / d_bh: the gas and black-hole slot arrays PI indexes (nsph, nbh slots); all 8-byte aligned device memory,
 * counts below 2^31 - 64.  A workgroup stages 256 records in LDS with 16-byte loads, works on them there and streams the tile back if
 * a loop changed it; the slots are written per particle.  With INIT, a pass before it checks the PI of every Type-0 and Type-5 particle:
 * one outside its slot array is SHQ_ERR_INVALID with nothing written.  A Type above 5 with Mass == 0 counts in badmass and keeps its
 * mass (the reference reads past MassTable); it enters mass_total only.  The sums are reproducible: wave and block partial sums in
 * a fixed shape, then one fixed-order pass over the block sums.  The conditions the reference ends the run on are reported, the call
 * returns SHQ_OK.  Synchronous (the report crosses PCIe). */
int shq_startup_particles(shq_context *ctx, const shq_startup_layout *layout, void *d_parts, int64_t numpart, void *d_sph, int64_t nsph, void *d_bh, int64_t nbh,
                          const shq_startup_params *params, int which, shq_startup_report *report);
/* check_density_entropy over the slot array itself: Density <= 0 or not finite becomes meanbar (counted in *bad), EgyWtDensity <= 0 or
 * not finite becomes Density, Entropy below GAMMA_MINUS1 MinEgySpec / pow(Density / atime^3, GAMMA_MINUS1) is raised to it. */
int shq_startup_check_density_entropy(shq_context *ctx, const shq_startup_layout *layout, void *d_sph, int64_t nsph, double meanbar, double MinEgySpec, double atime,
                                      int64_t *bad);

/* set_init_hsml for the resident particles (shq_particles_upload with Type and flags, Hsml resident) and the current tree, which must
 * carry the particle -> leaf array (shq_tree_build, or shq_tree_upload of a tree with father): Type 0 and 5 particles that are not
 * garbage climb from their leaf while 10 DesNumNgb Mass > the node's mass and get len pow(3 / (4 pi) DesNumNgb Mass / mass, 1 / 3) of
 * the node they end on when that is below 500 MeanGasSeparation, else MeanGasSeparation; a particle the tree does not hold (a swallowed
 * black hole) keeps no = its own index and gets MeanGasSeparation.  d_node_out (device, int32 per particle, may be NULL): that node,
 * numbered from the tree's firstnode as the caller's NODE array is (for a device-built tree: shq_tree_download with firstnode =
 * NumPart), the particle's own index when it never entered the tree, -1 for particles the loop skips.  The reference's conditions
 * "Bad tree moments" (len > BoxSize - which the root, 1.001 BoxSize long, meets - or node mass < Mass), "Bad hsml guess" (Hsml <= 0)
 * and "Bad init father" (here: a father chain longer than 64) are counted; any of them is SHQ_ERR_INVALID after every Hsml has
 * been written. */
int shq_set_init_hsml(shq_context *ctx, double MeanGasSeparation, double DesNumNgb, int32_t *d_node_out);
/* Entropy = GAMMA_MINUS1 u_init / pow(X / a3, GAMMA_MINUS1) for every resident gas particle, X = EgyWtDensity (from_egywt, which also
 * keeps X for shq_setup_smoothinglengths' max-change reduction) or Density; GAMMA_MINUS1 = (5.0 / 3.0) - 1. */
int shq_init_entropy(shq_context *ctx, double u_init, double a3, int from_egywt);

typedef struct shq_startup_sml_params {
    shq_density_params density;   /* update_hsml and DoEgyDensity are set by the call */
    double MeanGasSeparation, u_init, atime;
    int32_t DensityIndependentSphOn;
    int32_t pad_;
} shq_startup_sml_params;
typedef struct shq_startup_sml_stats {
    shq_sph_stats first;          /* the density pass with update_hsml */
    int32_t nrounds;              /* entropy + density rounds of setup_density_indep_entropy (0 without DensityIndependentSph) */
    int32_t nmaxdiff;             /* rounds that were followed by the max-change reduction: nrounds - 1 when the loop stopped, else 100 */
    double maxdiff[100];
    int64_t nbad_moments, nbad_hsml; /* set_init_hsml's "Bad tree moments" and "Bad hsml guess" particles: reported, the call goes on */
} shq_startup_sml_stats;
/* setup_smoothinglengths for RestartSnapNum == -1 on host views: one upload, then on the device the GASMASK + BHMASK tree,
 * shq_set_init_hsml, density with update_hsml = 1 and DoEgyDensity = 0, and either the entropy from Density or
 * setup_density_indep_entropy's loop (EgyWtDensity = Density; entropy, density with DoEgyDensity = 1, max over gas of
 * |EgyWtDensity - old| / EgyWtDensity; one more round after the max falls below 1e-3, 100 at most); then one write-back of Hsml,
 * DtHsml, Density, EgyWtDensity, DhsmlEgyDensityFactor, DivVel, CurlVel, Entropy and the black-hole slots for the walked targets, as
 * shq_density_close does (Hsml also for the particles set_init_hsml wrote and no walk visits: a swallowed black hole).  No tree stays installed.  No gas and no black-hole slots: SHQ_OK, nothing done.  SHQ_ERR_NOCONV passes through.
 * Particles that meet set_init_hsml's conditions (in a set so small or so sparse that a climb reaches the root) are counted in the
 * stats and the call goes on with the Hsml they got, which the density loop then corrects; the reference ends the run there. */
int shq_setup_smoothinglengths(shq_context *ctx, const shq_part_view *parts, const shq_sph_view *sph, const shq_bh_view *bh, const shq_startup_sml_params *params,
                               shq_startup_sml_stats *stats);

/* ---- Run logs: energy statistics, black-hole totals and details (libgadget/stats.cpp:217-396, bhinfo.cpp:66-204; csrc/stats.hip) ---------
 * The particle loops behind the run's log files, on device-resident records in the conventions of shq_io_* / shq_startup_*: records are
 * opaque device bytes, fields are byte offsets, results arrive in host structs, the calls are synchronous.  Records and slots are read only.
 *   compute_global_quantities_of_system's loop (stats.cpp:235-272)      shq_energy_statistics   device records
 *   its rank-0 block (:289-361)                                         shq_stats_finish        host
 *   write_blackhole_txt's loop (bhinfo.cpp:176-184)                     shq_bh_totals           device slots
 *   collect_BH_info's loop (:76-151)                                    shq_bh_details          device records, slots and BHPriv arrays
 * The all-reduce between the loops and the lines, and the files, stay with the caller. */
typedef struct shq_stats_layout {
    /* double Pos[3], float Mass, the Type byte, int32 PI, double Vel[3], double Potential: the rules of shq_startup_layout (8-byte aligned
     * records of a multiple of 8 and at most 240 bytes, every member inside and aligned to its own size) */
    size_t part_elsize, off_pos, off_mass, off_type, off_pi, off_vel, off_potential;
    /* gas slot (a multiple of 8, at most 480 bytes): doubles Density, Entropy, Ne; local_J21 and zreion may be SHQ_NOFIELD */
    size_t sph_elsize, sph_off_density, sph_off_entropy, sph_off_ne, sph_off_local_j21, sph_off_zreion;
} shq_stats_layout;
typedef struct shq_stats_params {
    double Time;
    int32_t want_temperature;          /* 0: no get_temp solves, TemperatureComp stays 0, no cooling tables needed */
    int32_t uvbg_mode;                 /* SHQ_COOL_UVBG_*; the members below as in shq_cooling_step; redshift = 1 / Time - 1 */
    shq_cooling_uvbg GlobalUVBG;
    double CurrentParticleOffset[3];
    double J21_coeffs[6];
    double ss_greyopac_factor, ss_fbar_factor;
} shq_stats_params;
typedef struct shq_stats_sums {        /* the rank's raw sums, struct state_of_system's Comp members before MPI_Reduce */
    double MassComp[6], EnergyPotComp[6], EnergyKinComp[6], EnergyIntComp[6];
    double TemperatureComp[6];         /* sum of Mass * T, not yet divided */
    double MomentumComp[6][4], AngMomentumComp[6][4], CenterOfMassComp[6][4];   /* column 3 is 0 */
    int64_t count[6];                  /* particles by type */
    int64_t n_bad_type;                /* Type > 5: the reference indexes past its arrays; here counted, adding nothing */
    int64_t n_status[SHQ_COOL_NSTATUS]; /* temperature solves by outcome */
    int64_t n_deferred;                /* entries the deferred list would hold: the solves that did not end SHQ_COOL_OK */
    double kernel_ms;                  /* HIP-event time from the first kernel to the last */
} shq_stats_sums;
typedef struct shq_stats_state {       /* struct state_of_system, stats.h */
    double Mass, EnergyKin, EnergyPot, EnergyInt, EnergyTot;
    double Momentum[4], AngMomentum[4], CenterOfMass[4];
    double MassComp[6], EnergyKinComp[6], EnergyPotComp[6], EnergyIntComp[6], EnergyTotComp[6], TemperatureComp[6];
    double MomentumComp[6][4], AngMomentumComp[6][4], CenterOfMassComp[6][4];
} shq_stats_state;
/* stats.cpp:235-272 statement by statement, f64 without contraction: a1, a2, a3 = Time, Time * Time, Time * Time * Time; Mass widened from
 * float; no garbage or swallowed test, as the reference has none.  For gas egyspec = Entropy / GAMMA_MINUS1 * pow(Density / a3,
 * GAMMA_MINUS1) and T = get_temp(Density, egyspec, 1 - HYDROGEN_MASSFRAC, &uvbg, &ne): density and energy enter the rate network in
 * internal units, as the reference passes them (the units of shq_cooling_set_tables are not applied); ne starts from the slot's Ne and
 * is not written back; uvbg is get_local_UVBG as in shq_cooling (the Zreion table is that of shq_cooling_set_tables).  A solve that does
 * not end SHQ_COOL_OK adds nothing to TemperatureComp[0], is counted in n_status, and its particle index goes to `deferred` (host,
 * index order): the contract of the deferred lists; more than deferred_capacity of them is SHQ_ERR_NOMEM after everything else has been
 * written.  The sums are reproducible: a wave adds each type its ballot holds in one butterfly, the wave sums are added in wave order,
 * and a second kernel adds the block sums in a fixed order; no floating-point atomics.  One pass over the records (256-record tiles staged
 * in LDS, as in shq_startup_particles); the temperature solves run in a second kernel over the list of gas particles.
 * SHQ_ERR_STATE when temperatures are wanted without shq_cooling_set_tables, or in the Zreion mode without a Zreion table;
 * SHQ_ERR_INVALID for a broken layout, the J21 mode with local_J21 or zreion SHQ_NOFIELD, or a gas PI outside [0, nsph) (tested on the
 * device before the slot is read); in each case no output is touched. */
int shq_energy_statistics(shq_context *ctx, const shq_stats_layout *layout, const void *d_parts, int64_t numpart, const void *d_sph, int64_t nsph,
                          const shq_stats_params *params, shq_stats_sums *out, int32_t *deferred, int64_t deferred_capacity);
/* Rank 0's block on sums the caller has added over the ranks, in the reference's expression order: EnergyTotComp, TemperatureComp /
 * MassComp where MassComp > 0, the totals, the centres of mass divided by their mass, the [3] norms.  No GPU. */
int shq_stats_finish(const shq_stats_sums *summed, shq_stats_state *out);

/* write_blackhole_txt's loop over the nbh black-hole slots at d_bh (bh_elsize bytes each, a multiple of 8, at most 480; uint64 SwallowID,
 * doubles Mass and Mdot): the slots with SwallowID == (uint64) -1 add to *num and to sums[] = { Mass, Mdot, Mdot / Mass }.  Reproducible
 * as above. */
int shq_bh_totals(shq_context *ctx, const void *d_bh, int64_t nbh, size_t bh_elsize, size_t off_swallowid, size_t off_mass, size_t off_mdot, int64_t *num,
                  double sums[3]);

#define SHQ_BHINFO_SIZE 436   /* sizeof(struct BHinfo), packed, MyFloat a double; size1 = size2 = 428 */
typedef struct shq_bh_detail_layout {
    /* particle record: double Pos[3], float Mass, the flag byte (bit 1 Swallowed), the Type byte, int32 PI, double Vel[3],
     * double FullTreeGravAccel[3], uint64 ID */
    size_t part_elsize, off_pos, off_mass, off_flags, off_type, off_pi, off_vel, off_fulltreegravaccel, off_id;
    /* black-hole slot: doubles Mass, Mdot, Density, Mtrack, KineticFdbkEnergy, VDisp, DFAccel[3], DF_SurroundingVel[3], DF_SurroundingRmsVel,
     * DF_SurroundingDensity, DragAccel[3], MinPot, MinPotPos[3]; unsigned char minTimeBin, char encounter, uint64 SwallowID, int32 CountProgs */
    size_t bh_elsize, bh_off_mintimebin, bh_off_encounter, bh_off_mass, bh_off_mdot, bh_off_density, bh_off_mtrack, bh_off_kineticfdbkenergy, bh_off_vdisp,
        bh_off_dfaccel, bh_off_df_surroundingvel, bh_off_df_surroundingrmsvel, bh_off_df_surroundingdensity, bh_off_dragaccel, bh_off_swallowid, bh_off_minpot,
        bh_off_minpotpos, bh_off_countprogs;
} shq_bh_detail_layout;
typedef struct shq_bh_detail_arrays {   /* struct BHPriv's arrays, device memory, by black-hole slot; a NULL array leaves its members zero */
    const double *BH_Entropy, *BH_SurroundingGasVel /* [][3] */, *BH_accreted_momentum /* [][3] */, *BH_accreted_Mass, *BH_accreted_BHMass,
        *BH_FeedbackWeightSum, *NumDM, *MgasEnc;
    const int32_t *KEflag;
    const uint64_t *SPH_SwallowID;      /* indexed by the black hole's own PI, as the reference does */
    int64_t n_sph_swallowid;            /* its length (the reference sizes it by the gas slots); the other arrays hold nbh entries */
    double CurrentParticleOffset[3];    /* subtracted from Pos and MinPotPos */
} shq_bh_detail_arrays;
/* collect_BH_info's loop: d_out (device) receives nactive records of SHQ_BHINFO_SIZE bytes in the reference's packed format, record k for
 * particle d_active[k] (device; NULL: particle k).  BH_SurroundingParticles and V1sumDM stay zero.  A record is composed as 109 32-bit
 * words and stored word by word.  SHQ_ERR_INVALID, tested on the device before the dependent read, the output then unspecified: an
 * active index outside [0, numpart) (the reference's test lets numpart through), a Type other than 5, a PI outside [0, nbh) or, with
 * SPH_SwallowID given, outside [0, n_sph_swallowid). */
int shq_bh_details(shq_context *ctx, const shq_bh_detail_layout *layout, const void *d_parts, int64_t numpart, const void *d_bh, int64_t nbh,
                   const shq_bh_detail_arrays *arrays, const int32_t *d_active, int64_t nactive, double atime, void *d_out);

#ifdef __cplusplus
}
#endif
#endif /* SHENQI_HIP_H */
