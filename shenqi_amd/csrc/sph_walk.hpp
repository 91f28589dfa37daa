/* sph_walk.hpp — the device side every neighbour-walk kernel shares: the SPH kernels, SphDev, the per-lane neighbour lists and the
 * three walks (ngb_walk: 64 targets per wave; heavy_walk: one target per wave; heavy_block: one target per workgroup), and the
 * host helpers of sph.hip that the operator files (sph_ngbsums.hip, sph_bh.hip, sph_winds.hip) drive their walks with.
 * For .hip files only: everything device-side is a template or __forceinline__ in an anonymous namespace, so each including
 * file instantiates exactly the walks its own kernels use.  No __global__ kernel lives here. */
#pragma once
#include "common.hpp"
#include <math.h>
#include <stdlib.h>

#define SPH_GAMMA (5.0 / 3.0)      /* physconst.h:35 */
#define SPH_GAMMA_MINUS1 (SPH_GAMMA - 1)
#define SPH_MAXITER 400            /* treewalk2.h:21 */

namespace {

__device__ __forceinline__ double wrapd(double d, double L, double invL) { return fma(-L, rint(d * invL), d); }

/* Price (2012) kernels as libgadget/densitykernel.hpp:28-178 defines them (integer powers
 * written as products). KT: 1 cubic, 2 quintic, 4 quartic. */
template <int KT> struct Kern {
    static constexpr double support = (KT == 1) ? 4.0 : ((KT == 2) ? 6.0 : 5.0);
    double H, Wknorm, dnorm;
    __device__ __forceinline__ explicit Kern(double H_) : H(H_)
    {
        const double sigma = (KT == 1) ? (1 / M_PI) : ((KT == 2) ? (1 / (120 * M_PI)) : (1 / (20 * M_PI)));
        const double s = support / 2. / H;
        Wknorm = sigma * (s * s * s);
        dnorm = Wknorm * support / 2. / H;
    }
    static __device__ __forceinline__ double p3(double x) { return x * x * x; }
    static __device__ __forceinline__ double p4(double x) { const double y = x * x; return y * y; }
    static __device__ __forceinline__ double p5(double x) { const double y = x * x; return y * y * x; }
    __device__ __forceinline__ double wk_int(double q) const
    {
        if(KT == 1) {
            if(q < 1.0) return 0.25 * p3(2 - q) - p3(1 - q);
            if(q < 2.0) return 0.25 * p3(2 - q);
            return 0.0;
        } else if(KT == 4) {
            if(q < 0.5) return p4(2.5 - q) - 5 * p4(1.5 - q) + 10 * p4(0.5 - q);
            if(q < 1.5) return p4(2.5 - q) - 5 * p4(1.5 - q);
            if(q < 2.5) return p4(2.5 - q);
            return 0.0;
        } else {
            if(q < 1.0) return p5(3 - q) - 6 * p5(2 - q) + 15 * p5(1 - q);
            if(q < 2.0) return p5(3 - q) - 6 * p5(2 - q);
            if(q < 3.0) return p5(3 - q);
            return 0.0;
        }
    }
    __device__ __forceinline__ double dwk_int(double q) const
    {
        if(KT == 1) {
            if(q < 1.0) return -0.25 * 3 * (2 - q) * (2 - q) + 3 * (1 - q) * (1 - q);
            if(q < 2.0) return -0.25 * 3 * (2 - q) * (2 - q);
            return 0.0;
        } else if(KT == 4) {
            if(q < 0.5) return -4 * p3(2.5 - q) + 20 * p3(1.5 - q) - 40 * p3(0.5 - q);
            if(q < 1.5) return -4 * p3(2.5 - q) + 20 * p3(1.5 - q);
            if(q < 2.5) return -4 * p3(2.5 - q);
            return 0.0;
        } else {
            if(q < 1.0) return -5 * p4(3 - q) + 30 * p4(2 - q) - 75 * p4(1 - q);
            if(q < 2.0) return -5 * p4(3 - q) + 30 * p4(2 - q);
            if(q < 3.0) return -5 * p4(3 - q);
            return 0.0;
        }
    }
    __device__ __forceinline__ double wk(double u) const { return Wknorm * wk_int(u * support / 2.); }
    __device__ __forceinline__ double dwk(double u) const { return dnorm * dwk_int(u * support / 2.); }
    __device__ __forceinline__ double volume() const { return (4.0 / 3 * M_PI) * (H * H * H); }
};

/* everything the hydro pair evaluation reads of a neighbour, in ONE 128-byte line (round 4: position and mass moved in, in the place of
 * the padding and of the EntVarPred copy next to the velocity: eight 16-byte gathers per pair instead of ten — the evaluation kernel is
 * bound by the texture addresser's cycles per gather instruction, not by arithmetic) */
struct alignas(128) HydRec {
    double4 posm; /* x, y, z, mass */
    double4 velh; /* predicted velocity, Hsml */
    double4 C;    /* EntVarPred, density_j, soundspeed_j, p_over_rho2_j */
    double4 D;    /* Dhsml_j, rr2_j, f2_j, dloga_for_bin_j */
};
static_assert(sizeof(HydRec) == 128, "HydRec must be one 128-byte line");

struct SphDev {
    /* node pool */
    const NodeB *nodeB;
    const NodeC *nodeC;
    double *hmax;               /* per node */
    const int32_t *pfather;     /* particle -> packed father leaf */
    int root;
    int npool;                  /* packed nodes */
    /* leaf-order neighbour data */
    const double4 *posm_leaf;   /* x,y,z,m */
    const double4 *velp_leaf;   /* predicted velocity, EntVarPred */
    const HydRec *hydrec_leaf;  /* one 128-byte line per neighbour for the hydro pair evaluation */
    const double *hsml_leaf;
    const int32_t *flag_leaf;   /* bit0 skip (garbage / not gas), bit1 wind-decoupled */
    const float4 *posf_leaf;    /* f32 pre-test copy: x, y, z rounded; w = pre32_bound(Hsml); x = NaN: skip, x = inf: never accepted */
    const int32_t *ngarb_leaf;  /* at a leaf's first slot: how many of its particles are to be skipped (x = NaN above) */
    /* per particle */
    const double4 *posm;
    const uint8_t *pflags;
    double *hsml;
    double *dthsml;
    const double4 *velp;
    const double4 *hydC;
    const double4 *hydD;
    /* density scratch / outputs, by particle index */
    double *numngb, *dhsmldens, *left, *right;
    double *rho, *egyrho, *dhsmlegy, *div, *curl;
    double *rot;      /* [N][3] */
    double *gradrho;  /* [N][3] or null */
    /* hydro outputs */
    double *hacc;     /* [N][3] */
    double *dtent, *maxsig;
    double Box, invBox;
    /* targets too heavy even for a wave of their own: handed on to the one-target-per-workgroup kernel */
    int32_t *heavy2;
    long long *nheavy2;
};

/* ---- the f32 pre-test of the candidate scan (round 4) ----------------------------------------------------------------
 * The scan of a candidate tile tests ~2500 candidates per wave, of which a lane is interested in a tenth and accepts a
 * twentieth, in f64: 3 subtractions, 3 multiply-adds and a compare at four cycles each.  On gfx950 the f32 VOP2 forms issue at
 * twice that rate, and the decision does not have to be exact THERE: the lists may hold a superset as long as the evaluation
 * applies the reference's own test to every entry (it recomputes r2 in f64 anyway).  So the scan runs on coordinates rounded
 * to f32 (error <= 2^-24 |x| each, <= 2^-22 Box on a displacement with room to spare) against the bound
 * (h + 2^-20 Box)^2 (1 + 2^-20) rounded up: r < h in f64 implies the f32 test passes.  For h / Box = 3e-3 (1024^3) the lists
 * grow by 0.1 %.  Leaves whose displacements may need the periodic wrap keep the f64 scan (their tile does). */
__device__ __forceinline__ float pre32_bound(double h, double eps)
{
    const double b = (h + eps) * (h + eps) * (1.0 + 0x1p-20);
    float f = (float) b;
    if((double) f < b)
        f = __uint_as_float(__float_as_uint(f) + 1u); /* b > 0 and finite: the next float up */
    return f;
}

/* ---- density walk ------------------------------------------------------------------------------ */
/* Per-lane neighbour lists.  The union walk hands every leaf particle to all lanes whose search
 * sphere touches the leaf, but only a few of them actually have it within their kernel support; doing
 * the pair arithmetic (~100 f64 instructions for density, ~200 for hydro) under that mask keeps 10-20 %
 * of the lanes busy.  So the walk only runs the distance test (a dozen instructions) and appends the
 * accepted leaf slot to the lane's list; at the end of the walk (or when a list is full) every lane
 * works through ITS OWN list with vector loads, all lanes busy.  A lane meets its neighbours in exactly
 * the order of the depth-first walk, so sums are bit-identical to the immediate evaluation.
 * A lane collects its ~100 neighbours in a burst while the walk passes its corner of the group's
 * volume, so short LDS lists flushed whenever one lane fills up ran 431 pair rounds per wave for 112
 * pairs per target; the lists therefore live in global memory (L2-resident scratch, one region per
 * resident wave of a persistent grid, [entry][lane] so appends and reads coalesce) and are long enough
 * to be drained once. */
#define NL_CAP 256      /* list entries per lane; quintic-kernel neighbourhoods hold ~113, symmetric hydro lists up to ~200 */
#define NL_ROWS (NL_CAP + 64) /* rows of a wave's list region: a lane's fill is checked against NL_CAP once per candidate tile (<= 64 appends) */
#define NL_MAXBLOCKS 4096 /* persistent workgroups (4 waves each) that own a list region */

template <class F> __device__ __forceinline__ void nl_flush(const int32_t *myl, int &fill, F &&pair)
{
    int s_next = fill > 0 ? myl[0] : 0;
    for(int j = 0; shq_ballot(j < fill) != 0ull; j++) {
        const int s = s_next;
        if(j + 1 < fill)
            s_next = myl[(j + 1) * 64]; /* in flight while this pair is evaluated */
        if(j < fill)
            pair(s);
    }
    fill = 0;
}

/* ---- the neighbour walk shared by density and hydro ------------------------------------------------
 * Same wavefront-collective union walk as before (wave-uniform `cur`, per-lane `mynext`, cull_node per
 * lane), restructured around LDS so that no step waits on a dependent global load per node or per
 * candidate (with 4 waves per SIMD those ~1000-cycle waits kept the VALUs 44 % busy):
 *   - node window: the pool is in depth-first pre-order and a walk mostly moves forward in it, so the
 *     wave fetches 64 consecutive node records at a time (coalesced) into LDS and reads the node under
 *     the cursor from there; a jump outside the window reloads it;
 *   - candidate tile: leaves some lane wants are queued (slot range + the mask of interested lanes);
 *     when 64 candidates are queued the wave gathers them in ONE coalesced load, parks position, Hsml
 *     and flag in LDS, and every lane runs the distance test over the tile with broadcast reads;
 *   - accepted candidates go to the lane's list (see above) and are evaluated lane by lane.
 * Leaves are queued and tiles are scanned in walk order, so each lane still meets its neighbours in
 * depth-first order. */
#ifndef SPH_NODE_SCALAR
#define SPH_NODE_SCALAR 0 /* 1: the walk reads the node under its cursor with scalar loads instead of from an LDS window (A/B knob) */
#endif
#ifndef SPH_PROBE
#define SPH_PROBE 0 /* timing probes of the walk kernels (tools/sph_ab.sh with build_variant.sh): never in a shipped build */
#endif
#ifndef SPH_LEAF_ASM
#define SPH_LEAF_ASM 1 /* the walk-only kernels (KEEP) fetch the PRE32 scan's leaf records by inline-asm scalar loads straight into the
                          carried registers; 0: the compiler's loads everywhere (A/B knob).  tests/test_leaf_asm_isa_cpu.py reads the ISA
                          of those kernels and fails if the compiler ever copies or spills the registers while the loads travel */
#endif
#ifndef SPH_WALK_WPB
#define SPH_WALK_WPB 1 /* waves per block of the walk-only kernels (MODE 1) */
#endif
#define NW_WIN 32 /* nodes per window: half a window costs a few more reloads and buys 1.8 KB of LDS per wave */
/* per wave: node window (centre + len, links, hmax for the symmetric cull) and candidate tile (position, interested
 * lanes per queued leaf, leaf records, slot with the two flag bits on top, Hsml for the symmetric test): 4.5 KB (density) / 5.4 KB (hydro), so
 * that the walk kernels reach 7-8 waves per SIMD instead of 5 */
#define NW_LDS_PER_WAVE(SYM) (NW_WIN * (32 + 16 + ((SYM) ? 8 : 0)) + 64 * (32 + 8 + 4 + 4 + ((SYM) ? 8 : 0)))

/* KEEP: only build the lists (two-kernel path): nothing is evaluated, `fill` returns the list length, and a
 * lane whose list would overflow sets `ovf` (its wave is then redone by the fused kernel). */
/* GHOSTS (LocalNgbTreeWalk::visit<TREEWALK_GHOSTS>, localtreewalk2.h:378-437): an imported query walks only the branches
 * under the top-level nodes of its NodeList = the pre-order index ranges [start, sibling(start)); `seg` holds the (sorted)
 * packed start indices.  As in the gravity walk a lane waits at the start of its next branch and the wave cursor, which
 * still begins at the root, also descends wherever a lane waits further down. */
/* PRE32: tiles none of whose leaves may need the periodic wrap are scanned with the f32 pre-test (pre32_bound above; thri = the
 * target's own bound); `pair` must then apply the exact test itself. */
template <bool SYM, bool KEEP, bool GHOSTS, bool PRE32 = false, class Accept, class Pair>
__device__ __forceinline__ unsigned int ngb_walk(const SphDev &a, char *lds_wave, int32_t *myl, const bool valid, const double px,
                                                 const double py, const double pz, const double h, Accept &&accept, Pair &&pair,
                                                 unsigned int *dbg, int &fill, bool &ovf, const int4 seg = make_int4(-1, -1, -1, -1),
                                                 const float thri = 0.f)
{
    double4 *winB = reinterpret_cast<double4 *>(lds_wave);
    int4 *winC = reinterpret_cast<int4 *>(lds_wave + NW_WIN * 32);
    double *winH = reinterpret_cast<double *>(lds_wave + NW_WIN * 48); /* SYM only */
    char *tl = lds_wave + NW_WIN * (SYM ? 56 : 48);
    double4 *tq = reinterpret_cast<double4 *>(tl);
    unsigned long long *lqm = reinterpret_cast<unsigned long long *>(tl + 64 * 32); /* per queued LEAF: the lanes that want it */
    int *tsl = reinterpret_cast<int *>(tl + 64 * 40);                  /* leaf slot | flags << 30 once gathered */
    int *lqi = reinterpret_cast<int *>(tl + 64 * 44);                  /* per queued leaf: first candidate | count << 8 | may-wrap << 16 */
    double *th = reinterpret_cast<double *>(tl + 64 * 48);             /* SYM only */
    const int lane = threadIdx.x & 63;
    const double halfBox = 0.5 * a.Box;
    unsigned int nint = 0;
    int ncand = 0, nleafq = 0;
    fill = 0;
    ovf = false;
    int mynext = valid ? a.root : -2;
    /* PRE32: the leaf waiting for its f32 records (scalar loads: a leaf's records are consecutive and the same for every lane, so
     * they travel through the scalar cache into scalar registers: no LDS tile, no gather, no vector register) */
    typedef const float __attribute__((address_space(4))) *FloatK;
    typedef const int32_t __attribute__((address_space(4))) *IntK;
    typedef __attribute__((address_space(1))) char *GChar;
    typedef const double __attribute__((address_space(4))) *DoubleK;
    const DoubleK nodeBK = (DoubleK) (size_t) a.nodeB, hmaxK = (DoubleK) (size_t) a.hmax;
    const IntK nodeCK = (IntK) (size_t) a.nodeC;
    (void) nodeBK; (void) hmaxK; (void) nodeCK;
    const FloatK posfK = (FloatK) (size_t) a.posf_leaf;
    auto ldrec = [&](const int slot) { return make_float4(posfK[4 * slot], posfK[4 * slot + 1], posfK[4 * slot + 2], posfK[4 * slot + 3]); };
    const IntK ngarbK = (IntK) (size_t) a.ngarb_leaf;
    const float pfx = (float) px, pfy = (float) py, pfz = (float) pz;
    GChar region = nullptr; /* the wave's list region as a scalar base: an append is one store with a 32-bit lane offset */
    if(PRE32) {
        const unsigned long long rb = (unsigned long long) (myl - lane);
        region = (GChar) (size_t) (((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (rb >> 32)) << 32) |
                                   (unsigned) __builtin_amdgcn_readfirstlane((int) rb));
    }
    int p_cn = 0, p_sb = 0, p_ng = 0;
    unsigned long long p_km = 0ull;
    /* KEEP (the walk-only kernels of the two-kernel path): the waiting leaf's records by inline-asm scalar loads straight into the
     * loop-carried registers, waited for in process_pending.  The compiler's own loads go through temporaries and are waited for and
     * copied at the join (s_waitcnt lgkmcnt(0) + a column of s_mov right behind the loads): nothing travelled while the walk went on.
     * The asm hides the loads from the compiler, so nothing may copy or spill those registers between the loads and the wait: true of
     * the walk-only kernels (checked on their ISA by tests/test_leaf_asm_isa_cpu.py at every build of the test suite), not of the fused
     * kernels, whose evaluation code makes the allocator spill scalars: those keep the compiler's loads. */
    constexpr bool LEAF_ASM = SPH_LEAF_ASM && KEEP && !GHOSTS;
    typedef float f4s __attribute__((ext_vector_type(4)));
    f4s pd0, pd1, pd2, pd3, pd4, pd5, pd6, pd7;
    pd0 = pd1 = pd2 = pd3 = pd4 = pd5 = pd6 = pd7 = (f4s) (0.f);

    /* scan the queued candidates: one coalesced gather, then broadcast reads.  Leaf by leaf (round 4): what is the same for a leaf's
     * particles - which lanes want it, whether a displacement to it can need the periodic wrap at all - is read once per leaf into
     * scalar registers (the interested lanes become the lane condition through an inverse ballot: no vector instruction), and a lane's
     * fill is checked against NL_CAP once per tile (the list region has 64 rows of slack) instead of once per candidate:
     * 22 -> 13 vector instructions per candidate, the same candidates in the same order with the same accept decisions. */
    auto scan_tile = [&]() {
        if(lane < ncand) {
            const int s = tsl[lane];
            tq[lane] = a.posm_leaf[s];
            tsl[lane] = s | (a.flag_leaf[s] << 30);
            if(SYM)
                th[lane] = a.hsml_leaf[s];
        }
        __builtin_amdgcn_wave_barrier();
        for(int L = 0; L < nleafq; L++) {
            const int info = __builtin_amdgcn_readfirstlane(lqi[L]);
            const unsigned long long kmv = lqm[L];
            const unsigned long long kms = ((unsigned long long) (unsigned) __builtin_amdgcn_readfirstlane((int) (kmv >> 32)) << 32) |
                                           (unsigned) __builtin_amdgcn_readfirstlane((int) kmv);
            const int c0 = info & 0xff, cn = (info >> 8) & 0xff;
            const bool maywrap = (info >> 16) != 0;
            /* what holds for the whole leaf: the lane wants it and has not left the walk (a lane leaves at a tile's end only) */
            const bool keepL = __builtin_amdgcn_inverse_ballot_w64(kms) && !(KEEP && ovf);
            /* the candidate's slot and flags are the same in every lane: scalar registers, and a garbage particle (rare) is passed
             * over by a scalar branch instead of a lane condition; eight copies of the body with compile-time LDS offsets */
#pragma unroll
            for(int k = 0; k < SHQ_NMAXCHILD; k++) {
                if(k >= cn)
                    break;
                const int sf = __builtin_amdgcn_readfirstlane(tsl[c0 + k]), s = sf & 0x3fffffff, fl = (int) ((unsigned) sf >> 30);
                if(fl & 1)
                    continue;
                const double4 q = tq[c0 + k];
                const double hj = SYM ? th[c0 + k] : 0.0;
                double d0 = px - q.x, d1 = py - q.y, d2 = pz - q.z;
                if(maywrap) { /* wave-uniform; wrapping a displacement that does not need it is the identity */
                    d0 = wrapd(d0, a.Box, a.invBox);
                    d1 = wrapd(d1, a.Box, a.invBox);
                    d2 = wrapd(d2, a.Box, a.invBox);
                }
                const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
                if(keepL) {
                    nint++;
                    if(accept(r2, hj, fl)) {
                        myl[fill * 64] = s;
                        fill++;
                    }
                }
            }
        }
        if(KEEP) {
            if(fill >= NL_CAP) { /* this target's list does not fit: it leaves the walk (the others' lists stay good) and is
                                    walked on its own by a whole wave afterwards (heavy_walk) */
                ovf = true;
                fill = 0;
                mynext = -2;
            }
        } else if(shq_ballot(fill >= NL_CAP) != 0ull) {
            if(dbg)
                dbg[2] += NL_CAP;
            nl_flush(myl, fill, pair);
        }
        if(dbg)
            dbg[1] += ncand;
        __builtin_amdgcn_wave_barrier();
        ncand = 0;
        nleafq = 0;
    };

    /* PRE32: the f32 pre-test of the waiting leaf's candidates, straight-line code per leaf size; the candidates are scalar operands */
    auto process_pending = [&]() {
        if(p_cn == 0 || (SPH_PROBE == 1 && SYM)) /* probe 1: the hydro walk without its candidates */
            return;
        if(LEAF_ASM)
            asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(pd0), "+s"(pd1), "+s"(pd2), "+s"(pd3), "+s"(pd4), "+s"(pd5), "+s"(pd6), "+s"(pd7), "+s"(p_ng));
        if(__builtin_amdgcn_inverse_ballot_w64(p_km) && !(KEEP && ovf)) { /* the lane mask of the whole leaf */
            nint += p_cn - p_ng;
            unsigned int off = ((unsigned int) fill * 64u + (unsigned int) lane) * 4u;
#if SPH_PROBE == 2 /* timing probe: the hydro walk's tests without the list (the lists stay empty) */
#define PRE32_STORE(k)                                                                                                                  \
    if(SYM)                                                                                                                             \
        nint++;                                                                                                                         \
    else {                                                                                                                              \
        *reinterpret_cast<__attribute__((address_space(1))) int32_t *>(region + off) = p_sb + (k);                                      \
        off += 256u;                                                                                                                    \
    }
#else
#define PRE32_STORE(k)                                                                                                                  \
    *reinterpret_cast<__attribute__((address_space(1))) int32_t *>(region + off) = p_sb + (k);                                          \
    off += 256u;
#endif
#define PRE32_BODY(k, Q)                                                                                                                \
    {                                                                                                                                   \
        const float e0 = pfx - Q.x, e1 = pfy - Q.y, e2 = pfz - Q.z;                                                                     \
        const float rr = e0 * e0 + e1 * e1 + e2 * e2;                                                                                   \
        if(rr < (SYM ? fmaxf(thri, Q.w) : thri)) {                                                                                      \
            PRE32_STORE(k)                                                                                                              \
        }                                                                                                                               \
    }
            switch(p_cn) {
            case 1: PRE32_BODY(0, pd0) break;
            case 2: PRE32_BODY(0, pd0) PRE32_BODY(1, pd1) break;
            case 3: PRE32_BODY(0, pd0) PRE32_BODY(1, pd1) PRE32_BODY(2, pd2) break;
            case 4: PRE32_BODY(0, pd0) PRE32_BODY(1, pd1) PRE32_BODY(2, pd2) PRE32_BODY(3, pd3) break;
            case 5: PRE32_BODY(0, pd0) PRE32_BODY(1, pd1) PRE32_BODY(2, pd2) PRE32_BODY(3, pd3) PRE32_BODY(4, pd4) break;
            case 6: PRE32_BODY(0, pd0) PRE32_BODY(1, pd1) PRE32_BODY(2, pd2) PRE32_BODY(3, pd3) PRE32_BODY(4, pd4) PRE32_BODY(5, pd5) break;
            case 7: PRE32_BODY(0, pd0) PRE32_BODY(1, pd1) PRE32_BODY(2, pd2) PRE32_BODY(3, pd3) PRE32_BODY(4, pd4) PRE32_BODY(5, pd5) PRE32_BODY(6, pd6) break;
            default: PRE32_BODY(0, pd0) PRE32_BODY(1, pd1) PRE32_BODY(2, pd2) PRE32_BODY(3, pd3) PRE32_BODY(4, pd4) PRE32_BODY(5, pd5) PRE32_BODY(6, pd6) PRE32_BODY(7, pd7) break;
            }
#undef PRE32_BODY
            fill = (int) (off >> 8); /* lane * 4 < 256 */
        }
        if(dbg)
            dbg[1] += p_cn;
        p_cn = 0;
        if(KEEP) {
            if(fill >= NL_CAP) { /* as in scan_tile; checked per leaf here (<= 8 appends, the region has 64 rows of slack) */
                ovf = true;
                fill = 0;
                mynext = -2;
            }
        } else if(shq_ballot(fill >= NL_CAP) != 0ull) {
            if(dbg)
                dbg[2] += NL_CAP;
            nl_flush(myl, fill, pair);
        }
    };

    int seg1 = -1, seg2 = -1, seg3 = -1, myend = -1;
    if(GHOSTS) {
        mynext = (valid && seg.x >= 0) ? seg.x : -2;
        seg1 = seg.y; seg2 = seg.z; seg3 = seg.w;
        if(mynext >= 0)
            myend = a.nodeC[mynext].sibling;
    }
    int cur = a.root, wbase = -(1 << 30);
    /* The loop is written for the scalar pipe (round 4; the counter pass had 69 k scalar beside 56 k vector instructions per wave, and a
     * scalar instruction holds its pipe for four cycles like an f64 one): lane conditions exist only as ballot masks, combined with
     * 64-bit scalar algebra and read back through inverse ballots; wave-uniform decisions are compare-and-branch on those masks,
     * never booleans the compiler would materialise as masks of their own; one window test; the lanes' links are set before the
     * leaf is handed on, so that nothing after the hand-over depends on it. */
    while(cur >= 0) {
#if SPH_NODE_SCALAR
        /* the node under the cursor through the scalar cache into scalar registers (as the gravity walk reads its nodes): no LDS window,
         * no refills, no read-first-lanes; the tests take the record's fields as scalar operands */
        const double4 B = make_double4(nodeBK[4 * (size_t) cur], nodeBK[4 * (size_t) cur + 1], nodeBK[4 * (size_t) cur + 2], nodeBK[4 * (size_t) cur + 3]);
        const int Csib = nodeCK[4 * (size_t) cur], Cchild = nodeCK[4 * (size_t) cur + 1];
        const int Ctype = nodeCK[4 * (size_t) cur + 2], Ccount = nodeCK[4 * (size_t) cur + 3];
        const double Hnode = SYM ? hmaxK[(size_t) cur] : 0.0;
#else
        if((unsigned int) (cur - wbase) >= (unsigned int) NW_WIN) {
            wbase = cur;
            __builtin_amdgcn_wave_barrier();
            if(lane < NW_WIN) {
                const int idx = min(cur + lane, a.npool - 1);
                const NodeB nb = a.nodeB[idx];
                const NodeC nc = a.nodeC[idx];
                winB[lane] = make_double4(nb.center[0], nb.center[1], nb.center[2], nb.len);
                winC[lane] = make_int4(nc.sibling, nc.child, nc.type, nc.count);
                if(SYM)
                    winH[lane] = a.hmax[idx];
            }
            __builtin_amdgcn_wave_barrier();
        }
        const int w = cur - wbase;
        const double4 B = winB[w];
        const int4 Cv = winC[w];
        const int Csib = __builtin_amdgcn_readfirstlane(Cv.x), Cchild = __builtin_amdgcn_readfirstlane(Cv.y);
        const int Ctype = __builtin_amdgcn_readfirstlane(Cv.z), Ccount = __builtin_amdgcn_readfirstlane(Cv.w);
        const double Hnode = SYM ? winH[w] : 0.0;
#endif
        if(dbg)
            dbg[0]++;
        /* cull_node<symmetric>, localtreewalk2.h:154-182 */
        const unsigned long long actm = shq_ballot(mynext == cur);
        const double dist = (SYM ? fmax(Hnode, h) : h) + 0.5 * B.w;
        double dx = B.x - px, dy = B.y - py, dz = B.z - pz;
        double dmax = fmax(fmax(fabs(dx), fabs(dy)), fabs(dz));
        const unsigned long long wrapm = shq_ballot(dmax > halfBox) & actm;
        if(wrapm != 0ull) {
            dx = wrapd(dx, a.Box, a.invBox);
            dy = wrapd(dy, a.Box, a.invBox);
            dz = wrapd(dz, a.Box, a.invBox);
            dmax = fmax(fmax(fabs(dx), fabs(dy)), fabs(dz));
        }
        asm volatile("" ::: "memory");
        const double r2 = dx * dx + dy * dy + dz * dz;
        const double dist2 = dist + (0.5 * (1.7320508075688772 - 1.0)) * B.w;
        const unsigned long long keepm = actm & ~(shq_ballot(dmax > dist) | shq_ballot(r2 > dist2 * dist2));
        /* the node types without control flow: every awake lane passes on to the sibling; the lanes that keep an internal node go down
         * instead, and the cursor with them; a kept leaf is the one branch */
        unsigned long long openm = Ctype == SHQ_NODE_NODE_TYPE ? keepm : 0ull;
        const unsigned long long leafm = (Ctype == SHQ_PARTICLE_NODE_TYPE && Ccount > 0) ? keepm : 0ull;
        unsigned long long downm = openm;
        if(GHOSTS) /* a lane waits at a branch below this node: go down even if nobody opens it */
            downm |= Ctype == SHQ_NODE_NODE_TYPE ? shq_ballot(mynext > cur && (Csib < 0 || mynext < Csib)) : 0ull;
        if(__builtin_amdgcn_inverse_ballot_w64(actm))
            mynext = Csib;
        if(__builtin_amdgcn_inverse_ballot_w64(openm))
            mynext = Cchild;
        const int next = downm != 0ull ? Cchild : Csib;
        asm volatile("" ::: "memory");
        if(leafm != 0ull) {
            if(!PRE32 && ncand + Ccount > 64)
                scan_tile();
            /* can a displacement from an interested lane to a particle of this leaf need the periodic wrap?  The particles lie in
             * the leaf's cell: |p - pos| <= |centre - pos| + len / 2 per coordinate; no, unless the node test itself wrapped or
             * that bound comes near Box / 2 for some interested lane (a conservative yes costs three identity wraps) */
            const unsigned long long nearm = wrapm | (shq_ballot(dmax + 0.5 * B.w > 0.999 * halfBox) & leafm);
            if(PRE32)
                process_pending(); /* leaves are scanned in walk order: the waiting one first */
            if(PRE32 && nearm == 0ull) {
                /* this leaf waits for its records while the walk goes on */
                if(LEAF_ASM) {
                    const FloatK rp = posfK + 4 * (size_t) Cchild;
                    const IntK gp = ngarbK + (size_t) Cchild;
                    asm volatile("s_load_dwordx4 %0, %9, 0x0\n\ts_load_dwordx4 %1, %9, 0x10\n\ts_load_dwordx4 %2, %9, 0x20\n\t"
                                 "s_load_dwordx4 %3, %9, 0x30\n\ts_load_dwordx4 %4, %9, 0x40\n\ts_load_dwordx4 %5, %9, 0x50\n\t"
                                 "s_load_dwordx4 %6, %9, 0x60\n\ts_load_dwordx4 %7, %9, 0x70\n\ts_load_dword %8, %10, 0x0"
                                 : "=&s"(pd0), "=&s"(pd1), "=&s"(pd2), "=&s"(pd3), "=&s"(pd4), "=&s"(pd5), "=&s"(pd6), "=&s"(pd7), "=&s"(p_ng)
                                 : "s"(rp), "s"(gp));
                } else {
                    auto ld4 = [&](const int slot) { const float4 r = ldrec(slot); f4s v; v.x = r.x; v.y = r.y; v.z = r.z; v.w = r.w; return v; };
                    pd0 = ld4(Cchild); pd1 = ld4(Cchild + 1); pd2 = ld4(Cchild + 2); pd3 = ld4(Cchild + 3);
                    pd4 = ld4(Cchild + 4); pd5 = ld4(Cchild + 5); pd6 = ld4(Cchild + 6); pd7 = ld4(Cchild + 7);
                    p_ng = ngarbK[Cchild];
                }
                p_km = leafm;
                p_sb = Cchild;
                p_cn = Ccount;
            } else {
                if(lane < Ccount)
                    tsl[ncand + lane] = Cchild + lane;
                if(lane == 0) {
                    lqm[nleafq] = leafm;
                    lqi[nleafq] = ncand | (Ccount << 8) | ((nearm != 0ull ? 1 : 0) << 16);
                }
                nleafq++;
                ncand += Ccount;
                if(PRE32)
                    scan_tile(); /* a leaf that may need the periodic wrap: the f64 scan, at once */
            }
        }
        if(GHOSTS) {
            if(shq_ballot(mynext == myend) & actm) { /* rare: some lane's branch is done */
                if(__builtin_amdgcn_inverse_ballot_w64(actm) && mynext == myend) { /* wait at the next one of the NodeList */
                    mynext = seg1 >= 0 ? seg1 : -2;
                    seg1 = seg2;
                    seg2 = seg3;
                    seg3 = -1;
                    myend = mynext >= 0 ? a.nodeC[mynext].sibling : -1;
                }
            }
        }
        cur = next;
    }
    if(PRE32)
        process_pending();
    if(ncand > 0)
        scan_tile();
    if(dbg) {
        int mf = fill;
        for(int off = 32; off > 0; off >>= 1)
            mf = max(mf, __shfl_xor(mf, off));
        dbg[2] += mf;
    }
    if(!KEEP)
        nl_flush(myl, fill, pair);
    return nint;
}

/* ---- one target, one wave --------------------------------------------------------------------------------------
 * A target whose neighbour list outgrows NL_CAP (gas next to a density caustic: the kernel-weighted count reaches its
 * target only when the support sphere already holds thousands of particles near its rim) would keep one lane busy for
 * as many rounds as it has neighbours while the other 63 idle.  Such targets are taken out of the group walks and each
 * gets a wave to itself, with the lanes on the work instead of on targets: node rounds pop up to 64 nodes of an LDS
 * stack and cull them one per lane (cull_node, localtreewalk2.h:154-182, against the one target), kept leaves queue
 * their particle slots, and candidate rounds take 64 queued particles, one per lane, through the same accept / pair
 * code; the lanes' partial sums are added across the wave at the end.  Same neighbour set and candidate count as the
 * group walk; the sum runs in a different order (rounding-level differences). */
#define HW_STACK 1024
#define HW_SOFT 512   /* above this fill the walk goes depth-first, one node per round: at most 7 more per tree level */
#define HW_UNR 4      /* candidates per lane and candidate round (round 4): the round's gathers are independent loads in flight together */
#define HW_CAND (64 * HW_UNR + 64 * 8 + 64) /* < 64 HW_UNR pending + <= 64 x 8 queued per node round */
#define HW_LDS ((HW_STACK + HW_CAND) * 4)

#define HW_ABORT 16384 /* candidates after which a wave gives its target up to a whole workgroup (heavy_block) */

template <bool SYM, class Accept, class Pair>
__device__ __forceinline__ unsigned int heavy_walk(const SphDev &a, char *lds_wave, const double px, const double py, const double pz,
                                                   const double h, Accept &&accept, Pair &&pair, bool &aborted)
{
    int *stk = reinterpret_cast<int *>(lds_wave);
    int *cq = stk + HW_STACK;
    const int lane = threadIdx.x & 63;
    unsigned int nint = 0;
    int S = 1, nc = 0, chead = 0, done = 0;
    aborted = false;
    if(lane == 0)
        stk[0] = a.root;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for(;;) {
        if(nc >= 64 * HW_UNR || (S == 0 && nc > 0)) {
            /* candidate round: up to HW_UNR candidates per lane, their records requested together (a round used to be one dependent
             * gather of 64 records: a target with 10^4 candidates spent its time waiting for 160 of them, one after the other) */
            const int m = nc < 64 * HW_UNR ? nc : 64 * HW_UNR;
            int sj[HW_UNR], flj[HW_UNR];
            double4 qj[HW_UNR];
            double hjj[HW_UNR];
#pragma unroll
            for(int j = 0; j < HW_UNR; j++) {
                const int idx = lane + 64 * j;
                sj[j] = -1;
                flj[j] = 1;
                qj[j] = make_double4(0, 0, 0, 0);
                hjj[j] = 0.0;
                if(idx < m) {
                    const int s = cq[(chead + idx) % HW_CAND];
                    sj[j] = s;
                    qj[j] = a.posm_leaf[s];
                    flj[j] = a.flag_leaf[s];
                    hjj[j] = SYM ? a.hsml_leaf[s] : 0.0;
                }
            }
#pragma unroll
            for(int j = 0; j < HW_UNR; j++)
                if(sj[j] >= 0 && !(flj[j] & 1)) {
                    nint++;
                    const double4 q = qj[j];
                    const double d0 = wrapd(px - q.x, a.Box, a.invBox), d1 = wrapd(py - q.y, a.Box, a.invBox), d2 = wrapd(pz - q.z, a.Box, a.invBox);
                    if(accept(d0 * d0 + d1 * d1 + d2 * d2, hjj[j], flj[j]))
                        pair(sj[j]);
                }
            chead = (chead + m) % HW_CAND;
            nc -= m;
            done += m;
            if(done > HW_ABORT && a.heavy2) {
                aborted = true;
                return 0;
            }
            __builtin_amdgcn_wave_barrier();
        } else if(S > 0) {
            /* node round */
            int k = S < 64 ? S : 64;
            const int room = (HW_SOFT - S) / 7;
            if(room < k)
                k = room > 1 ? room : 1;
            const bool on = lane < k;
            const int node = on ? stk[S - 1 - lane] : 0;
            S -= k;
            __builtin_amdgcn_wave_barrier();
            bool keep = false;
            NodeC nc4;
            nc4.sibling = nc4.child = -1;
            nc4.type = SHQ_PSEUDO_NODE_TYPE;
            nc4.count = 0;
            if(on) {
                const NodeB nb = a.nodeB[node];
                nc4 = a.nodeC[node];
                const double dist = (SYM ? fmax(a.hmax[node], h) : h) + 0.5 * nb.len;
                const double dx = wrapd(nb.center[0] - px, a.Box, a.invBox), dy = wrapd(nb.center[1] - py, a.Box, a.invBox),
                             dz = wrapd(nb.center[2] - pz, a.Box, a.invBox);
                const double dmax = fmax(fmax(fabs(dx), fabs(dy)), fabs(dz));
                const double r2 = dx * dx + dy * dy + dz * dz;
                const double dist2 = dist + (0.5 * (1.7320508075688772 - 1.0)) * nb.len;
                keep = !(dmax > dist) && !(r2 > dist2 * dist2);
            }
            /* kept leaves queue their particle slots */
            const bool leaf = keep && nc4.type == SHQ_PARTICLE_NODE_TYPE;
#pragma unroll
            for(int j = 0; j < SHQ_NMAXCHILD; j++) {
                const bool has = leaf && j < nc4.count;
                const unsigned long long msk = shq_ballot(has);
                if(msk == 0ull)
                    break;
                if(has)
                    cq[(chead + nc + __builtin_amdgcn_mbcnt_hi((unsigned) (msk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) msk, 0u))) % HW_CAND] =
                        nc4.child + j;
                nc += __popcll(msk);
            }
            /* kept internal nodes push their children: the first one, then along the sibling links up to the node's own sibling */
            int c = (keep && nc4.type == SHQ_NODE_NODE_TYPE) ? nc4.child : -1;
            for(int j = 0; j < 8; j++) {
                const bool has = c >= 0 && c != nc4.sibling;
                const unsigned long long msk = shq_ballot(has);
                if(msk == 0ull)
                    break;
                if(has) {
                    const int at = S + __builtin_amdgcn_mbcnt_hi((unsigned) (msk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) msk, 0u));
                    if(at < HW_STACK)
                        stk[at] = c;
                    c = a.nodeC[c].sibling;
                }
                S += __popcll(msk);
            }
            if(S > HW_STACK) { /* deeper than the slack allows (64 levels): stop rather than walk a truncated stack; the sums come out wrong and
                                  the Hsml loop reports non-convergence */
                S = 0;
                nc = 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else
            break;
    }
    return nint;
}

__device__ __forceinline__ double wave_sum(double v)
{
    for(int off = 32; off > 0; off >>= 1)
        v += __shfl_xor(v, off);
    return v;
}

/* ---- one target, one workgroup of 8 waves: the same walk for the few targets whose support sphere holds a good part of a
 * dense clump (10^5 - 10^6 candidates: a wave alone would need tens of milliseconds).  Stack and candidate queue are shared
 * in LDS; every position comes from prefix sums over the thread index, so which thread meets which candidate — and with it
 * the order of the sum — is fixed: results are reproducible run to run. */
#define HB_THREADS 512
#define HB_WAVES (HB_THREADS / 64)
#define HB_STACK 8192
#define HB_SOFT 4096
#define HB_UNR 4 /* candidates per thread and candidate round, as HW_UNR */
#define HB_CAND (HB_THREADS * (8 + HB_UNR) + HB_THREADS)

struct HbShared {
    int stk[HB_STACK];
    int cq[HB_CAND];
    int wtot[2][HB_WAVES];
    double red[HB_WAVES];
    int S, nc, chead;
};

/* exclusive prefix over the threads of the workgroup of a count in [0, 8]; total to all */
__device__ __forceinline__ int hb_scan8(int v, int *wtot, int &total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long b0 = shq_ballot((v & 1) != 0), b1 = shq_ballot((v & 2) != 0), b2 = shq_ballot((v & 4) != 0), b3 = shq_ballot((v & 8) != 0);
    auto mb = [](unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((unsigned) (m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) m, 0u)); };
    const int pre = mb(b0) + 2 * mb(b1) + 4 * mb(b2) + 8 * mb(b3);
    if(lane == 0)
        wtot[wv] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2) + 8 * __popcll(b3);
    __syncthreads();
    int base = 0;
    total = 0;
    for(int w = 0; w < HB_WAVES; w++) {
        const int c = wtot[w];
        if(w < wv)
            base += c;
        total += c;
    }
    return base + pre;
}

__device__ __forceinline__ double hb_sum(double v, double *red)
{
    v = wave_sum(v);
    __syncthreads();
    if((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0;
    for(int w = 0; w < HB_WAVES; w++)
        t += red[w];
    return t;
}

__device__ __forceinline__ double hb_max(double v, double *red)
{
    for(int off = 32; off > 0; off >>= 1)
        v = fmax(v, __shfl_xor(v, off));
    __syncthreads();
    if((threadIdx.x & 63) == 0)
        red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
    for(int w = 1; w < HB_WAVES; w++)
        t = fmax(t, red[w]);
    return t;
}

template <bool SYM, class Accept, class Pair>
__device__ __forceinline__ unsigned int heavy_block(const SphDev &a, HbShared &sh, const double px, const double py, const double pz, const double h,
                                                    Accept &&accept, Pair &&pair)
{
    const int tid = threadIdx.x;
    unsigned int nint = 0;
    __syncthreads();
    if(tid == 0) {
        sh.stk[0] = a.root;
        sh.S = 1;
        sh.nc = 0;
        sh.chead = 0;
    }
    for(;;) {
        __syncthreads();
        const int S = sh.S, nc = sh.nc, chead = sh.chead;
        __syncthreads();
        if(nc >= HB_THREADS * HB_UNR || (S == 0 && nc > 0)) {
            const int m = nc < HB_THREADS * HB_UNR ? nc : HB_THREADS * HB_UNR;
            int sj[HB_UNR], flj[HB_UNR];
            double4 qj[HB_UNR];
            double hjj[HB_UNR];
#pragma unroll
            for(int j = 0; j < HB_UNR; j++) {
                const int idx = tid + HB_THREADS * j;
                sj[j] = -1;
                flj[j] = 1;
                qj[j] = make_double4(0, 0, 0, 0);
                hjj[j] = 0.0;
                if(idx < m) {
                    const int s = sh.cq[(chead + idx) % HB_CAND];
                    sj[j] = s;
                    qj[j] = a.posm_leaf[s];
                    flj[j] = a.flag_leaf[s];
                    hjj[j] = SYM ? a.hsml_leaf[s] : 0.0;
                }
            }
#pragma unroll
            for(int j = 0; j < HB_UNR; j++)
                if(sj[j] >= 0 && !(flj[j] & 1)) {
                    nint++;
                    const double4 q = qj[j];
                    const double d0 = wrapd(px - q.x, a.Box, a.invBox), d1 = wrapd(py - q.y, a.Box, a.invBox), d2 = wrapd(pz - q.z, a.Box, a.invBox);
                    if(accept(d0 * d0 + d1 * d1 + d2 * d2, hjj[j], flj[j]))
                        pair(sj[j]);
                }
            if(tid == 0) {
                sh.chead = (chead + m) % HB_CAND;
                sh.nc = nc - m;
            }
        } else if(S > 0) {
            int k = S < HB_THREADS ? S : HB_THREADS;
            const int room = (HB_SOFT - S) / 7;
            if(room < k)
                k = room > 1 ? room : 1;
            const bool on = tid < k;
            const int node = on ? sh.stk[S - 1 - tid] : 0;
            bool keep = false;
            NodeC nc4;
            nc4.sibling = nc4.child = -1;
            nc4.type = SHQ_PSEUDO_NODE_TYPE;
            nc4.count = 0;
            if(on) {
                const NodeB nb = a.nodeB[node];
                nc4 = a.nodeC[node];
                const double dist = (SYM ? fmax(a.hmax[node], h) : h) + 0.5 * nb.len;
                const double dx = wrapd(nb.center[0] - px, a.Box, a.invBox), dy = wrapd(nb.center[1] - py, a.Box, a.invBox),
                             dz = wrapd(nb.center[2] - pz, a.Box, a.invBox);
                const double dmax = fmax(fmax(fabs(dx), fabs(dy)), fabs(dz));
                const double r2 = dx * dx + dy * dy + dz * dz;
                const double dist2 = dist + (0.5 * (1.7320508075688772 - 1.0)) * nb.len;
                keep = !(dmax > dist) && !(r2 > dist2 * dist2);
            }
            const int cl = (keep && nc4.type == SHQ_PARTICLE_NODE_TYPE) ? nc4.count : 0;
            int kid[8], nk = 0;
            {
                int c = (keep && nc4.type == SHQ_NODE_NODE_TYPE) ? nc4.child : -1;
#pragma unroll
                for(int j = 0; j < 8; j++) {
                    const bool has = c >= 0 && c != nc4.sibling;
                    kid[j] = has ? c : -1;
                    if(has) {
                        nk++;
                        c = a.nodeC[c].sibling;
                    } else
                        c = -1;
                }
            }
            int totc = 0, totk = 0;
            const int offc = hb_scan8(cl, sh.wtot[0], totc); /* its barrier also orders the pops above before the pushes below */
            const int offk = hb_scan8(nk, sh.wtot[1], totk);
#pragma unroll
            for(int j = 0; j < 8; j++) {
                if(j < cl)
                    sh.cq[(chead + nc + offc + j) % HB_CAND] = nc4.child + j;
                if(j < nk && S - k + offk + j < HB_STACK)
                    sh.stk[S - k + offk + j] = kid[j];
            }
            if(tid == 0) {
                sh.nc = nc + totc;
                sh.S = (S - k + totk > HB_STACK) ? 0 : S - k + totk; /* deeper than the slack allows: stop (see heavy_walk) */
            }
        } else
            break;
    }
    return nint;
}

inline SphDev make_dev(shq_context *ctx, double Box)
{
    SphDev a;
    a.nodeB = ctx->nodeB.ptr;
    a.nodeC = ctx->nodeC.ptr;
    a.hmax = ctx->node_hmax.ptr;
    a.pfather = ctx->pfather.ptr;
    a.root = ctx->root;
    a.npool = (int) ctx->numnodes;
    a.posm_leaf = ctx->posm_leaf.ptr;
    a.velp_leaf = ctx->velp_leaf.ptr;
    a.hydrec_leaf = reinterpret_cast<const HydRec *>(ctx->hydrec_leaf.ptr);
    a.hsml_leaf = ctx->hsml_leaf.ptr;
    a.flag_leaf = ctx->flag_leaf.ptr;
    a.posf_leaf = ctx->posf_leaf.ptr;
    a.ngarb_leaf = ctx->ngarb_leaf.ptr;
    a.posm = ctx->posm.ptr;
    a.pflags = ctx->pflags.ptr;
    a.hsml = ctx->hsml.ptr;
    a.dthsml = ctx->dthsml.ptr;
    a.velp = ctx->velp.ptr;
    a.hydC = ctx->hydC.ptr;
    a.hydD = ctx->hydD.ptr;
    a.numngb = ctx->s_numngb.ptr;
    a.dhsmldens = ctx->s_dhsmldens.ptr;
    a.left = ctx->s_left.ptr;
    a.right = ctx->s_right.ptr;
    a.rho = ctx->g_density.ptr;
    a.egyrho = ctx->g_egywt.ptr;
    a.dhsmlegy = ctx->g_dhsmlegy.ptr;
    a.div = ctx->g_divvel.ptr;
    a.curl = ctx->g_curlvel.ptr;
    a.rot = ctx->s_rot.ptr;
    a.gradrho = nullptr;
    a.hacc = ctx->g_hydroaccel_out.ptr;
    a.dtent = ctx->g_dtentropy_out.ptr;
    a.maxsig = ctx->g_maxsignalvel.ptr;
    a.heavy2 = ctx->s_redo2.ptr;               /* null until a walk reserved it: the wave tier then never gives up */
    a.nheavy2 = ctx->s_counters.ptr ? ctx->s_counters.ptr + 7 : nullptr;
    a.Box = Box;
    a.invBox = 1.0 / Box;
    return a;
}

} // namespace

/* ---- host helpers, defined in sph.hip: the shared small kernels stay there, once, and the operator files reach them here ---- */
#define NL_REDO_BLOCKS 1024 /* workgroups of a fused walk: s_nlist2 holds one list region per wave of that many */

/* scratch of a bisection loop over a shrinking queue: s_numngb, s_left, s_right, s_todo, the two queue buffers, s_blockcount, s_counters */
int sph_reserve_redo(shq_context *ctx);
/* the list regions of one fused walk launch */
int sph_reserve_nlist2(shq_context *ctx);
/* x[0..n) = v (fill_kernel) */
void sph_fill(shq_context *ctx, double *d_x, long long n, double v);
/* velp and the skip flag in leaf order, Hsml by slot into d_hsml_leaf (sph_gather_leaf_kernel without hydro records, wind flag or f32 copy) */
void sph_gather_leaf_plain(shq_context *ctx, long long nl, double *d_hsml_leaf);
/* the flag of a leaf slot for walks over gas that is not garbage (bh_gather_leaf_kernel, sph_bh.hip); flag_leaf must hold the slots */
int sph_gather_gas_flags(shq_context *ctx);
/* order-preserving compaction of the `size` targets of the current queue whose s_todo entry is set, into `out`; *newsize = their
 * number (one host round trip: the stream is idle on return) */
int sph_compact_todo(shq_context *ctx, long long size, int32_t *out, long long *newsize);
/* stats of the walk timed between the SHQ_T_SPH events (one host round trip): d_nint[0] interactions; hmax_tried: d_nint[2] holds the
 * bits of the largest Hsml tried (the density loop), else hsml_max_tried = 0 */
int sph_fill_stats(shq_context *ctx, shq_sph_stats *stats, int64_t nq, int niter, const unsigned long long *d_nint, bool hmax_tried = false);

/* The bisection loop of stellar density and wind velocity dispersion: launch(cur, size, grid, ntasks) walks the current queue and
 * marks in s_todo who has to go again, the queue is compacted, until it is empty; more than SPH_MAXITER rounds: SHQ_ERR_NOCONV with
 * "failed to converge <what>".  `what` ends in a %lld for the number left. */
template <class Launch> int sph_redo_loop(shq_context *ctx, const int32_t *d_queue, long long nq, const char *what, Launch &&launch, int *niter)
{
    int32_t *bufs[2] = {ctx->s_queue2.ptr, ctx->s_queue3.ptr};
    int wsel = 0;
    const int32_t *cur = d_queue;
    long long size = nq;
    *niter = 0;
    while(size > 0) {
        const long long ntasks = (size + 255) / 256;
        launch(cur, size, (unsigned) (ntasks < NL_REDO_BLOCKS ? ntasks : NL_REDO_BLOCKS), ntasks);
        SHQ_HIP(hipGetLastError());
        (*niter)++;
        SHQ_TRY(sph_compact_todo(ctx, size, bufs[wsel], &size));
        cur = bufs[wsel];
        wsel ^= 1;
        if(size > 0 && *niter > SPH_MAXITER) {
            shq_set_error(what, size);
            return SHQ_ERR_NOCONV;
        }
    }
    return SHQ_OK;
}