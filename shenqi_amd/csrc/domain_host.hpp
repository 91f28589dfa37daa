/* domain_host.hpp — the serial stages of the domain decomposition as pure host C++ (no HIP, no context), restated from
 * libgadget/domain.cpp: the key automaton recovered from a key function, domain_toptree_merge, domain_global_refine,
 * domain_create_topleaves, domain_assign_topleaves_balanced, domain_set_task_leafs, domain_check_memory_bound, and the
 * renumbering of domain_toptree_garbage_collection.  domain.hip wraps them for the C-ABI; a stand-alone program may include this
 * header alone. */
#ifndef SHQ_DOMAIN_HOST_HPP
#define SHQ_DOMAIN_HOST_HPP

#include <algorithm>
#include <array>
#include <map>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/shenqi_hip.h"

namespace shq_domain_host {

/* ---- the key automaton ----------------------------------------------------------------------------------------------------- */

/* Signature of the octant path that ends at (x, y, z) after `depth` levels: the last digit of the key of every one-level and the last
 * two digits of every two-level continuation.  Paths with equal signatures continue alike (checked afterwards against keyfn). */
typedef std::array<uint8_t, 72> PeanoSig;
inline PeanoSig peano_signature(shq_peano_keyfn keyfn, int x, int y, int z, int depth)
{
    PeanoSig s;
    for(int o = 0; o < 8; o++)
        s[o] = (uint8_t) (keyfn((x << 1) | ((o >> 2) & 1), (y << 1) | ((o >> 1) & 1), (z << 1) | (o & 1), depth + 1) & 7);
    for(int o = 0; o < 64; o++) {
        const int xx = (x << 2) | (((o >> 5) & 1) << 1) | ((o >> 2) & 1);
        const int yy = (y << 2) | (((o >> 4) & 1) << 1) | ((o >> 1) & 1);
        const int zz = (z << 2) | (((o >> 3) & 1) << 1) | (o & 1);
        s[8 + o] = (uint8_t) (keyfn(xx, yy, zz, depth + 2) & 63);
    }
    return s;
}

inline uint64_t peano_key(const shq_peano_tables *t, int x, int y, int z, int bits)
{
    uint64_t key = 0;
    int s = 0;
    for(int b = bits - 1; b >= 0; b--) {
        const int o = (((x >> b) & 1) << 2) | (((y >> b) & 1) << 1) | ((z >> b) & 1);
        key = (key << 3) | t->sub[s][o];
        s = t->next[s][o];
    }
    return key;
}

/* 0 ok, 1 more than SHQ_PEANO_MAXSTATES states (or no closure within the depth a 21-bit key allows), 2 the tables do not reproduce keyfn */
inline int peano_tables_from_key(shq_peano_keyfn keyfn, shq_peano_tables *out)
{
    struct Rep { int x, y, z, depth; };
    memset(out, 0, sizeof(*out));
    std::map<PeanoSig, int> ids;
    std::vector<Rep> reps;
    ids[peano_signature(keyfn, 0, 0, 0, 0)] = 0;
    reps.push_back(Rep{0, 0, 0, 0});
    for(size_t s = 0; s < reps.size(); s++) {
        const Rep r = reps[s];
        if(r.depth + 3 > SHQ_PEANO_BITS)
            return 1;
        for(int o = 0; o < 8; o++) {
            const Rep c{(r.x << 1) | ((o >> 2) & 1), (r.y << 1) | ((o >> 1) & 1), (r.z << 1) | (o & 1), r.depth + 1};
            out->sub[s][o] = (uint8_t) (keyfn(c.x, c.y, c.z, c.depth) & 7);
            const PeanoSig sig = peano_signature(keyfn, c.x, c.y, c.z, c.depth);
            auto it = ids.find(sig);
            if(it == ids.end()) {
                if(reps.size() >= SHQ_PEANO_MAXSTATES)
                    return 1;
                it = ids.emplace(sig, (int) reps.size()).first;
                reps.push_back(c);
            }
            out->next[s][o] = (uint8_t) it->second;
        }
    }
    out->nstates = (int32_t) reps.size();
    /* the proof: the function itself, on triples the walk never saw (a 64-bit LCG; any fixed sequence does) */
    uint64_t g = 0x9E3779B97F4A7C15ull;
    for(int n = 0; n < 4096; n++) {
        int c[3];
        for(int d = 0; d < 3; d++) {
            g = g * 6364136223846793005ull + 1442695040888963407ull;
            c[d] = (int) ((g >> 33) & ((1u << SHQ_PEANO_BITS) - 1));
        }
        if(peano_key(out, c[0], c[1], c[2], SHQ_PEANO_BITS) != keyfn(c[0], c[1], c[2], SHQ_PEANO_BITS))
            return 2;
    }
    return 0;
}

inline bool peano_tables_ok(const shq_peano_tables *t)
{
    if(!t || t->nstates < 1 || t->nstates > SHQ_PEANO_MAXSTATES)
        return false;
    for(int s = 0; s < t->nstates; s++)
        for(int o = 0; o < 8; o++)
            if(t->next[s][o] >= t->nstates || t->sub[s][o] > 7)
                return false;
    return true;
}

/* ---- domain_toptree_garbage_collection (:919-943) ------------------------------------------------------------------------------
 * `nodes` are the survivors of the truncation in skeleton order, Daughter / Parent still skeleton indices, old[k] the skeleton index
 * of nodes[k] (ascending).  The reference moves the eight daughters of every surviving internal node to the front in depth-first
 * pre-order; the result is written to out (as many entries). */
inline void toptree_renumber(const std::vector<shq_local_topnode> &nodes, const std::vector<int32_t> &old, shq_local_topnode *out)
{
    auto pos_of = [&](int32_t skel) { return (int) (std::lower_bound(old.begin(), old.end(), skel) - old.begin()); };
    out[0] = nodes[0];
    out[0].Parent = -1;
    int last_free = 1;
    /* explicit stack of (new index) in the order the recursion visits them */
    std::vector<int> stack{0};
    while(!stack.empty()) {
        const int start = stack.back();
        stack.pop_back();
        if(out[start].Daughter < 0)
            continue;
        const int oldd = pos_of(out[start].Daughter), newd = last_free;
        out[start].Daughter = newd;
        last_free += 8;
        for(int j = 0; j < 8; j++) {
            out[newd + j] = nodes[(size_t) oldd + j];
            out[newd + j].Parent = start;
        }
        for(int j = 7; j >= 0; j--)
            stack.push_back(newd + j);
    }
}

/* ---- domain_toptree_merge (:1447-1552) ----------------------------------------------------------------------------------- */
inline int toptree_merge_r(shq_local_topnode *A, const shq_local_topnode *B, int noA, int noB, int *sizeA, int sizeB, int MaxTopNodes)
{
    if(B[noB].Shift < A[noA].Shift) {
        if(A[noA].Daughter < 0) {
            if(*sizeA + 8 > MaxTopNodes)
                return SHQ_ERR_RETRY;
            const int pb = B[noB].Parent;
            if(pb < 0 || pb >= sizeB)
                return SHQ_ERR_INVALID;
            const int64_t count = A[noA].Count - B[pb].Count;
            const int64_t cost = A[noA].Cost - B[pb].Cost;
            A[noA].Daughter = *sizeA;
            for(int j = 0; j < 8; j++) {
                shq_local_topnode &s = A[A[noA].Daughter + j];
                s.Shift = A[noA].Shift - 3;
                s.Count = (j + 1) * count / 8 - j * count / 8;
                s.Cost = (j + 1) * cost / 8 - j * cost / 8;
                s.Daughter = -1;
                s.Parent = noA;
                s.pad_ = 0;
                s.StartKey = A[noA].StartKey + (uint64_t) j * (1ull << s.Shift);
            }
            *sizeA += 8;
        }
        if(A[noA].Shift < 3)
            return SHQ_ERR_INVALID;
        const uint64_t oct = (B[noB].StartKey - A[noA].StartKey) >> (A[noA].Shift - 3);
        if(oct > 7)
            return SHQ_ERR_INVALID;
        return toptree_merge_r(A, B, A[noA].Daughter + (int) oct, noB, sizeA, sizeB, MaxTopNodes);
    }
    if(B[noB].Shift == A[noA].Shift) {
        A[noA].Count += B[noB].Count;
        A[noA].Cost += B[noB].Cost;
        if(B[noB].Daughter >= 0) {
            if(B[noB].Daughter + 8 > sizeB)
                return SHQ_ERR_INVALID;
            for(int j = 0; j < 8; j++) {
                const int sub = B[noB].Daughter + j;
                if(B[sub].Shift >= B[noB].Shift)
                    return SHQ_ERR_INVALID; /* "treeB is corrupt" */
                const int rc = toptree_merge_r(A, B, noA, sub, sizeA, sizeB, MaxTopNodes);
                if(rc != SHQ_OK)
                    return rc;
            }
        } else if(A[noA].Daughter >= 0) {
            for(int j = 0; j < 8; j++) {
                const int rc = toptree_merge_r(A, B, A[noA].Daughter + j, noB, sizeA, sizeB, MaxTopNodes);
                if(rc != SHQ_OK)
                    return rc;
            }
        }
        return SHQ_OK;
    }
    /* B is the larger cell: a spatial average into A, and on down A */
    const int diff = B[noB].Shift - A[noA].Shift;
    if(diff > 60)
        return SHQ_OK; /* "Refusing to merge two tree nodes of wildly different depth": n = 0 */
    const int64_t n = (int64_t) 1 << diff;
    A[noA].Count += B[noB].Count / n;
    A[noA].Cost += B[noB].Cost / n;
    if(A[noA].Daughter >= 0)
        for(int j = 0; j < 8; j++) {
            const int rc = toptree_merge_r(A, B, A[noA].Daughter + j, noB, sizeA, sizeB, MaxTopNodes);
            if(rc != SHQ_OK)
                return rc;
        }
    return SHQ_OK;
}

/* ---- domain_global_refine (:1320-1371) ------------------------------------------------------------------------------------ */
inline int global_refine(shq_local_topnode *T, int *size, int MaxTopNodes, int64_t countlimit, int64_t costlimit)
{
    for(int i = 0; i < *size; i++) {
        if(T[i].Daughter >= 0 || T[i].Shift <= 0)
            continue;
        if(T[i].Count < countlimit && T[i].Cost < costlimit)
            continue;
        if(*size + 8 > MaxTopNodes)
            return SHQ_ERR_RETRY;
        T[i].Daughter = *size;
        for(int j = 0; j < 8; j++) {
            shq_local_topnode &s = T[T[i].Daughter + j];
            s.Shift = T[i].Shift - 3;
            s.Count = T[i].Count / 8;
            s.Cost = T[i].Cost / 8;
            s.Daughter = -1;
            s.Parent = i;
            s.pad_ = 0;
            s.StartKey = T[i].StartKey + (uint64_t) j * (1ull << s.Shift);
        }
        *size += 8;
    }
    return SHQ_OK;
}

/* ---- domain_create_topleaves (:801-816): leaves numbered depth-first, daughters in key order ------------------------------- */
inline int create_topleaves(shq_topnode *N, int ntopnodes, shq_topleaf *L)
{
    int next = 0;
    std::vector<int> stack{0};
    while(!stack.empty()) {
        const int no = stack.back();
        stack.pop_back();
        if(N[no].Daughter == -1) {
            N[no].Leaf = next;
            L[next].topnode = no;
            next++;
        } else {
            if(N[no].Daughter <= no || N[no].Daughter + 8 > ntopnodes)
                return -1;
            for(int j = 7; j >= 0; j--)
                stack.push_back(N[no].Daughter + j);
        }
    }
    return next;
}

/* ---- domain_assign_topleaves_balanced (:619-761), NsegmentPerTask = 1 ------------------------------------------------------- */
struct LeafExt {
    uint64_t Key;
    int Task, topnode;
    int64_t cost;
};
inline int assign_topleaves_balanced(shq_topnode *N, shq_topleaf *L, int ntopleaves, const int64_t *cost, int NTask)
{
#pragma clang fp contract(off)
    const int Nsegment = NTask;
    std::vector<LeafExt> E((size_t) ntopleaves);
    for(int i = 0; i < ntopleaves; i++)
        E[i] = LeafExt{N[L[i].topnode].StartKey, -1, L[i].topnode, cost[i]};
    std::sort(E.begin(), E.end(), [](const LeafExt &a, const LeafExt &b) { return a.Key < b.Key; });
    int64_t totalcost = 0;
    for(int i = 0; i < ntopleaves; i++)
        totalcost += E[i].cost;
    int64_t totalcostLeft = totalcost;
    double mean_expected = 1.0 * totalcost / Nsegment;
    double mean_task = 1.0 * totalcost / NTask;
    int curleaf = 0, curseg = 0, curtask = 0, nrounds = 0;
    int64_t curload = 0, curtaskload = 0;
    while(nrounds < ntopleaves) {
        int append = 0, advance = 0;
        if(curleaf == ntopleaves) {
            advance = 1;
        } else if(ntopleaves - curleaf == Nsegment - curseg) {
            append = 1;
            advance = 1;
        } else {
            const int64_t totalassigned = (totalcost - totalcostLeft) + curload;
            if((mean_expected * (curseg + 1) - totalassigned > 0.5 * E[curleaf].cost) || curload == 0)
                append = 1;
            else
                advance = 1;
        }
        if(append) {
            curload += E[curleaf].cost;
            E[curleaf].Task = curtask;
            curleaf++;
        }
        if(advance) {
            curtaskload += curload;
            if((mean_task - curtaskload < 0.5 * mean_expected) || (Nsegment - curseg <= NTask - curtask)) {
                curtaskload = 0;
                curtask++;
            }
            totalcostLeft -= curload;
            curload = 0;
            curseg++;
            if(curtask == NTask) {
                curtask = 0;
                mean_expected = 1.0 * totalcostLeft / Nsegment;
                mean_task = 1.0 * totalcostLeft / NTask;
                nrounds++;
            }
            if(curleaf == ntopleaves)
                break;
        }
    }
    if(curseg < Nsegment || totalcostLeft != 0)
        return SHQ_ERR_INVALID; /* "Not enough segments were created" / "Total cost is not fully assigned" */
    std::sort(E.begin(), E.end(), [](const LeafExt &a, const LeafExt &b) { return a.Task != b.Task ? a.Task < b.Task : a.Key < b.Key; });
    for(int i = 0; i < ntopleaves; i++) {
        N[E[i].topnode].Leaf = i;
        L[i].Task = E[i].Task;
        L[i].topnode = E[i].topnode;
    }
    L[ntopleaves].Task = NTask;
    L[ntopleaves].topnode = -1;
    return SHQ_OK;
}

/* ---- domain_set_task_leafs (:764-793) --------------------------------------------------------------------------------------- */
inline int set_task_leafs(const shq_topleaf *L, int ntopleaves, int NTask, shq_task_leafs *Tasks)
{
    int ta = 0;
    Tasks[ta].StartLeaf = 0;
    for(int i = 0; i <= ntopleaves; i++) {
        if(L[i].Task == ta)
            continue;
        if(L[i].Task < ta || L[i].Task > NTask)
            return SHQ_ERR_INVALID;
        Tasks[ta].EndLeaf = i;
        ta++;
        while(ta < L[i].Task) {
            Tasks[ta].EndLeaf = i;
            Tasks[ta].StartLeaf = i;
            ta++;
        }
        Tasks[ta].StartLeaf = i;
    }
    return ta == NTask ? SHQ_OK : SHQ_ERR_INVALID;
}

/* ---- domain_check_memory_bound (:529-585) ---------------------------------------------------------------------------------- */
inline int check_memory_bound(const shq_task_leafs *Tasks, int NTask, const int64_t *TopLeafCount, int64_t MaxPart, double SetAsideFactor)
{
    int64_t max_load = 0;
    for(int ta = 0; ta < NTask; ta++) {
        int64_t load = 0;
        for(int i = Tasks[ta].StartLeaf; i < Tasks[ta].EndLeaf; i++)
            load += TopLeafCount[i];
        max_load = std::max(max_load, load);
    }
    return max_load > MaxPart * SetAsideFactor ? 1 : 0;
}

} // namespace shq_domain_host
#endif
