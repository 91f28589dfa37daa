/* domain.hip — the domain decomposition, domain_decompose_full (libgadget/domain.cpp:174-277), on the device.
 *
 *   PEANO()                                         utils/peano.h:15-21     shq_peano_keys
 *   domain_check_for_local_refine_subsample         domain.cpp:1005-1067    shq_domain_samples
 *     ... the skeleton loop, counts, truncation     :1073-1168, :892-958    shq_domain_local_toptree
 *   domain_compute_costs (counts)                   :1374-1429              shq_domain_leaf_counts
 *   the TopLeaf loop, layoutfunc                    :238-246, :159-164      shq_domain_particle_topleaves
 *   the serial stages (domain_host.hpp)                                     shq_domain_toptree_merge / _finish / _balance
 *
 * The key.  The library holds no Peano-Hilbert table: shq_peano_tables_from_key recovers the curve's automaton from a key function
 * the caller passes (domain_host.hpp).  The kernels read it from LDS as 16-bit entries (next << 6 | digits): 64 x 8 one-level entries
 * for the odd top bit, 64 x 64 two-level entries for the ten bit pairs below it, so a key is a chain of 11 dependent LDS reads.
 *
 * The skeleton has a closed form.  For sorted samples k[0..n), L[i] = leading octal digits (of 21) k[i-1] and k[i]
 * share, at most 20, L[0] = -1.  The serial loop splits, when it meets k[i], exactly the nodes at depths L[i-1]+1 .. L[i] on the path
 * of k[i], in that order, each split appending eight nodes.  So split number m = S[i] + (d - L[i-1] - 1) with S the exclusive scan of
 * max(0, L[i] - L[i-1]), its daughters are nodes 1 + 8 m .. 1 + 8 m + 7, and the node it splits is the root (d = 0), a daughter of
 * the previous split of the same sample (d > L[i-1] + 1), or a daughter of the split made when the second sample of the run that
 * shares the first d - 1 digits arrived (one binary search).  Count of any node = samples in its key range (two binary searches):
 * that is the leaf count and the sum up the tree at once.  Count == Cost and both fall monotonically down the tree, so the top-down
 * truncation keeps a node exactly when its parent's Count reaches min(countlimit, costlimit). */
#include "device_prims.hpp"
#include "domain_host.hpp"
#include <string.h>
#include <vector>

namespace {

namespace dh = shq_domain_host;

constexpr int DD_T1 = SHQ_PEANO_MAXSTATES * 8, DD_T2 = SHQ_PEANO_MAXSTATES * 64, DD_TAB = DD_T1 + DD_T2;

struct DdNode { /* struct topnode_data */
    unsigned long long StartKey;
    int32_t Daughter, Shift, Leaf, pad_;
};
static_assert(sizeof(DdNode) == sizeof(shq_topnode), "DdNode mirrors shq_topnode");
static_assert(sizeof(shq_local_topnode) == 40, "local_topnode_data is 40 bytes");

__device__ __forceinline__ void dd_load_tables(const uint16_t *__restrict__ g, uint16_t *lds)
{
    for(int k = threadIdx.x; k < DD_TAB / 2; k += blockDim.x)
        reinterpret_cast<uint32_t *>(lds)[k] = reinterpret_cast<const uint32_t *>(g)[k];
    __syncthreads();
}

/* PEANO(Pos, BoxSize), utils/peano.h:15-21 */
__device__ __forceinline__ unsigned long long dd_peano(const double *p, double Box, const uint16_t *lds)
{
#pragma clang fp contract(off)
    const double DomainFac = 1.0 / (Box * 1.001) * 2097152.0;
    const int ix = (int) ((p[0] + Box / 2000) * DomainFac), iy = (int) ((p[1] + Box / 2000) * DomainFac), iz = (int) ((p[2] + Box / 2000) * DomainFac);
    const int o = (((ix >> 20) & 1) << 2) | (((iy >> 20) & 1) << 1) | ((iz >> 20) & 1);
    unsigned e = lds[o]; /* state 0 */
    unsigned long long key = e & 7u;
    unsigned s = e >> 6;
#pragma unroll
    for(int b = 19; b >= 1; b -= 2) {
        const unsigned pix = (((ix >> b) & 1) << 5) | (((iy >> b) & 1) << 4) | (((iz >> b) & 1) << 3) | (((ix >> (b - 1)) & 1) << 2) | (((iy >> (b - 1)) & 1) << 1) |
                             ((iz >> (b - 1)) & 1);
        e = lds[DD_T1 + s * 64 + pix];
        key = (key << 6) | (e & 63u);
        s = e >> 6;
    }
    return key;
}

/* domain_get_topleaf, domain.h:69-76 (the installed tree is checked on the host: the walk ends within 21 steps inside the array) */
__device__ __forceinline__ int dd_topleaf(unsigned long long key, const DdNode *__restrict__ nodes)
{
    int no = 0;
    for(int l = 0; l < 22; l++) {
        const DdNode nd = nodes[no];
        if(nd.Daughter < 0)
            return nd.Leaf;
        no = nd.Daughter + (int) (((key - nd.StartKey) >> (nd.Shift - 3)) & 7ull);
    }
    return -1;
}

__global__ __launch_bounds__(256) void dd_keys_kernel(long long n, const char *__restrict__ pos, size_t stride, double Box, const uint16_t *__restrict__ tab,
                                                      unsigned long long *__restrict__ keys)
{
    __shared__ uint16_t lds[DD_TAB];
    dd_load_tables(tab, lds);
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    keys[i] = dd_peano(reinterpret_cast<const double *>(pos + (size_t) i * stride), Box, lds);
}

/* sample i of `nout` = slot i * dist: its key, PEANOCELLS for garbage; *nlive counts the live ones (one add per wave) */
__global__ __launch_bounds__(256) void dd_sample_keys_kernel(long long nout, long long dist, const char *__restrict__ parts, size_t elsize, size_t off_flags, size_t off_pos,
                                                             double Box, const uint16_t *__restrict__ tab, unsigned long long *__restrict__ keys,
                                                             unsigned long long *nlive)
{
    __shared__ uint16_t lds[DD_TAB];
    dd_load_tables(tab, lds);
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= nout)
        return;
    const char *p = parts + (size_t) (i * dist) * elsize;
    const bool garbage = *(const unsigned char *) (p + off_flags) & 1u;
    keys[i] = garbage ? SHQ_PEANOCELLS : dd_peano(reinterpret_cast<const double *>(p + off_pos), Box, lds);
    const unsigned long long live = __ballot(!garbage);
    if(live && (int) (threadIdx.x & 63) == __ffsll((long long) live) - 1)
        atomicAdd(nlive, (unsigned long long) __popcll(live));
}

__global__ void dd_stride_kernel(long long nout, long long dist, const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out)
{
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i < nout)
        out[i] = in[i * dist];
}

/* leading octal digits (of 21) two keys share, at most 20 */
__device__ __forceinline__ int dd_shared_digits(unsigned long long a, unsigned long long b)
{
    const unsigned long long x = a ^ b;
    if(!x)
        return 20;
    const int hb = 63 - __clzll((long long) x);
    const int t = 20 - hb / 3;
    return t < 0 ? -1 : t; /* bit 63 set: no sample key, nothing shared */
}
__device__ __forceinline__ int dd_L(const unsigned long long *__restrict__ k, long long i) { return i <= 0 ? -1 : dd_shared_digits(k[i - 1], k[i]); }

__global__ void dd_nsplit_kernel(long long n, const unsigned long long *__restrict__ k, long long *__restrict__ c)
{
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    const int d = dd_L(k, i) - dd_L(k, i - 1);
    c[i] = (i >= 1 && d > 0) ? d : 0;
}

struct DdSkel { /* the skeleton, one array per member: Daughter is written by the thread that splits the node, the rest by its parent's */
    unsigned long long *StartKey;
    int32_t *Daughter, *Parent, *Depth;
};

__global__ void dd_split_kernel(long long n, const unsigned long long *__restrict__ k, const long long *__restrict__ S, DdSkel sk, long long nnodes)
{
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i == 0) {
        sk.StartKey[0] = 0;
        sk.Parent[0] = -1;
        sk.Depth[0] = 0;
    }
    if(i < 1 || i >= n)
        return;
    const int L0 = dd_L(k, i - 1), L1 = dd_L(k, i);
    if(L1 <= L0)
        return;
    const unsigned long long key = k[i];
    long long m = S[i];
    long long node; /* the node at depth L0 + 1 on the path of key */
    if(L0 + 1 == 0)
        node = 0;
    else {
        /* depth L0 on the path was split when the second sample of the run sharing the first L0 digits arrived */
        const int dp = L0;
        const unsigned long long lo = dp == 0 ? 0ull : (key >> (3 * (21 - dp))) << (3 * (21 - dp));
        long long a = 0, e = i;
        while(a < e) {
            const long long mid = a + ((e - a) >> 1);
            if(k[mid] < lo)
                a = mid + 1;
            else
                e = mid;
        }
        const long long j = a + 1; /* <= i - 1: k[i-1] shares these digits too */
        const long long mp = S[j] + (dp - dd_L(k, j - 1) - 1);
        node = 1 + 8 * mp + (long long) ((key >> (3 * (20 - dp))) & 7ull);
    }
    for(int d = L0 + 1; d <= L1; d++, m++) {
        const long long first = 1 + 8 * m;
        if(node < 0 || node >= nnodes || first + 8 > nnodes)
            return; /* cannot happen for sorted keys; never write outside the arrays */
        sk.Daughter[node] = (int32_t) first;
        const int shift = 60 - 3 * d;
        const unsigned long long start = d == 0 ? 0ull : (key >> (shift + 3)) << (shift + 3);
        for(int j = 0; j < 8; j++) {
            sk.StartKey[first + j] = start + ((unsigned long long) j << shift);
            sk.Parent[first + j] = (int32_t) node;
            sk.Depth[first + j] = d + 1;
        }
        node = first + (long long) ((key >> shift) & 7ull);
    }
}

__device__ __forceinline__ long long dd_lower(const unsigned long long *__restrict__ k, long long n, unsigned long long v)
{
    long long a = 0, e = n;
    while(a < e) {
        const long long mid = a + ((e - a) >> 1);
        if(k[mid] < v)
            a = mid + 1;
        else
            e = mid;
    }
    return a;
}

__global__ void dd_count_kernel(long long nnodes, DdSkel sk, const unsigned long long *__restrict__ k, long long n, long long *__restrict__ count)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nnodes)
        return;
    const int shift = 63 - 3 * sk.Depth[t];
    const unsigned long long lo = sk.StartKey[t];
    const long long a = dd_lower(k, n, lo);
    const long long e = shift >= 63 ? n : dd_lower(k, n, lo + (1ull << shift));
    count[t] = e - a;
}

/* domain_toptree_truncate_r: a node goes when its parent's branch was cut, which (monotone counts) is when the parent itself is cheap */
__global__ void dd_flag_kernel(long long nnodes, DdSkel sk, const long long *__restrict__ count, long long lim, uint8_t *__restrict__ keep)
{
    const long long t = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(t >= nnodes)
        return;
    const int p = sk.Parent[t];
    keep[t] = (p < 0 || count[p] >= lim) ? 1 : 0;
}

__global__ void dd_gather_kernel(long long nkeep, const int32_t *__restrict__ list, DdSkel sk, const long long *__restrict__ count, long long lim,
                                 shq_local_topnode *__restrict__ out)
{
    const long long r = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(r >= nkeep)
        return;
    const int t = list[r];
    shq_local_topnode nd;
    nd.StartKey = sk.StartKey[t];
    nd.Shift = 63 - 3 * sk.Depth[t];
    nd.Daughter = (sk.Daughter[t] >= 0 && count[t] >= lim) ? sk.Daughter[t] : -1;
    nd.Parent = sk.Parent[t];
    nd.pad_ = 0;
    nd.Count = count[t];
    nd.Cost = count[t];
    out[r] = nd;
}

constexpr int DD_LDS_BINS = 8192;

/* domain_compute_costs with the thread-private tables as LDS bins per workgroup, folded with one 64-bit add per non-empty bin */
__global__ __launch_bounds__(256) void dd_leafcount_lds_kernel(long long n, const char *__restrict__ parts, size_t elsize, size_t off_flags, size_t off_pos, double Box,
                                                               const uint16_t *__restrict__ tab, const DdNode *__restrict__ nodes, int nleaves,
                                                               unsigned long long *__restrict__ counts)
{
    __shared__ uint16_t lds[DD_TAB];
    __shared__ unsigned int bins[DD_LDS_BINS];
    for(int b = threadIdx.x; b < nleaves; b += blockDim.x)
        bins[b] = 0;
    dd_load_tables(tab, lds);
    for(long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x) {
        const char *p = parts + (size_t) i * elsize;
        if(*(const unsigned char *) (p + off_flags) & 1u)
            continue;
        const int leaf = dd_topleaf(dd_peano(reinterpret_cast<const double *>(p + off_pos), Box, lds), nodes);
        if(leaf >= 0 && leaf < nleaves)
            atomicAdd(&bins[leaf], 1u);
    }
    __syncthreads();
    for(int b = threadIdx.x; b < nleaves; b += blockDim.x)
        if(bins[b])
            atomicAdd(&counts[b], (unsigned long long) bins[b]);
}

__global__ __launch_bounds__(256) void dd_leafcount_global_kernel(long long n, const char *__restrict__ parts, size_t elsize, size_t off_flags, size_t off_pos, double Box,
                                                                  const uint16_t *__restrict__ tab, const DdNode *__restrict__ nodes, int nleaves,
                                                                  unsigned long long *__restrict__ counts)
{
    __shared__ uint16_t lds[DD_TAB];
    dd_load_tables(tab, lds);
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    const char *p = parts + (size_t) i * elsize;
    if(*(const unsigned char *) (p + off_flags) & 1u)
        return;
    const int leaf = dd_topleaf(dd_peano(reinterpret_cast<const double *>(p + off_pos), Box, lds), nodes);
    if(leaf >= 0 && leaf < nleaves)
        atomicAdd(&counts[leaf], 1ull);
}

__global__ __launch_bounds__(256) void dd_particle_leaf_kernel(long long n, const char *__restrict__ parts, size_t elsize, size_t off_flags, size_t off_pos, double Box,
                                                               const uint16_t *__restrict__ tab, const DdNode *__restrict__ nodes, const int32_t *__restrict__ leaftask,
                                                               int nleaves, int32_t *__restrict__ topleaf, int32_t *__restrict__ target)
{
    __shared__ uint16_t lds[DD_TAB];
    dd_load_tables(tab, lds);
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i >= n)
        return;
    const char *p = parts + (size_t) i * elsize;
    if(*(const unsigned char *) (p + off_flags) & 1u) {
        if(target)
            target[i] = -1;
        return;
    }
    const int leaf = dd_topleaf(dd_peano(reinterpret_cast<const double *>(p + off_pos), Box, lds), nodes);
    topleaf[i] = leaf;
    if(target)
        target[i] = (leaf >= 0 && leaf < nleaves) ? leaftask[leaf] : -1;
}

/* the automaton as the kernels read it; uploaded when it differs from the one the context holds */
int use_tables(shq_context *ctx, const shq_peano_tables *t)
{
    SHQ_CHECK(dh::peano_tables_ok(t), SHQ_ERR_INVALID, "domain: the key tables are empty or name a state outside themselves (shq_peano_tables_from_key fills them)");
    if(ctx->dd_tab_valid && memcmp(&ctx->dd_tab_src, t, sizeof(*t)) == 0)
        return SHQ_OK;
    std::vector<uint16_t> h((size_t) DD_TAB, 0);
    for(int s = 0; s < t->nstates; s++)
        for(int o = 0; o < 8; o++) {
            h[(size_t) s * 8 + o] = (uint16_t) ((t->next[s][o] << 6) | t->sub[s][o]);
            const int s1 = t->next[s][o];
            for(int q = 0; q < 8; q++)
                h[(size_t) DD_T1 + (size_t) s * 64 + o * 8 + q] = (uint16_t) ((t->next[s1][q] << 6) | (t->sub[s][o] << 3) | t->sub[s1][q]);
        }
    SHQ_TRY(ctx->dd_tab.reserve((size_t) DD_TAB));
    ctx->dd_tab_valid = false;
    SHQ_HIP(hipMemcpyAsync(ctx->dd_tab.ptr, h.data(), sizeof(uint16_t) * h.size(), hipMemcpyHostToDevice, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* h lives on this frame */
    ctx->dd_tab_src = *t;
    ctx->dd_tab_valid = true;
    return SHQ_OK;
}

int check_parts(const shq_domain_parts *p)
{
    SHQ_CHECK(p && p->numpart >= 0 && p->numpart < (1ll << 31) - 64 && (p->d_parts || p->numpart == 0), SHQ_ERR_INVALID, "domain: bad particle array");
    SHQ_CHECK(p->elsize >= 24 && p->elsize % 8 == 0 && p->off_pos % 8 == 0 && p->off_pos + 24 <= p->elsize && p->off_flags < p->elsize, SHQ_ERR_INVALID,
              "domain: Pos must be three aligned doubles inside the record, the flag byte inside it");
    SHQ_CHECK(p->BoxSize > 0 && p->BoxSize < 1e300, SHQ_ERR_INVALID, "domain: BoxSize must be finite and positive");
    return SHQ_OK;
}

} // namespace

extern "C" int shq_peano_tables_from_key(shq_peano_keyfn keyfn, shq_peano_tables *out)
{
    SHQ_CHECK(keyfn && out, SHQ_ERR_INVALID, "null argument");
    const int rc = dh::peano_tables_from_key(keyfn, out);
    if(rc != 0)
        memset(out, 0, sizeof(*out));
    SHQ_CHECK(rc != 1, SHQ_ERR_INVALID, "peano_tables_from_key: more than %d states: the key function is no octant automaton of that size", SHQ_PEANO_MAXSTATES);
    SHQ_CHECK(rc != 2, SHQ_ERR_INVALID, "peano_tables_from_key: the recovered tables do not reproduce the key function at %d bits", SHQ_PEANO_BITS);
    return SHQ_OK;
}

extern "C" uint64_t shq_peano_key_host(const shq_peano_tables *tables, int x, int y, int z, int bits)
{
    if(!dh::peano_tables_ok(tables) || bits < 1 || bits > SHQ_PEANO_BITS)
        return ~0ull;
    return dh::peano_key(tables, x, y, z, bits);
}

extern "C" int shq_peano_keys(shq_context *ctx, const shq_peano_tables *tables, const void *d_pos, size_t stride_bytes, int64_t n, double BoxSize, uint64_t *d_keys)
{
    SHQ_CHECK(ctx && (n == 0 || (d_pos && d_keys)), SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(n >= 0 && stride_bytes >= 24 && stride_bytes % 8 == 0 && ((uintptr_t) d_pos % 8) == 0, SHQ_ERR_INVALID, "peano_keys: positions are three aligned doubles, stride a multiple of 8");
    SHQ_CHECK(BoxSize > 0 && BoxSize < 1e300, SHQ_ERR_INVALID, "peano_keys: BoxSize must be finite and positive");
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(use_tables(ctx, tables));
    if(n > 0) {
        dd_keys_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(n, (const char *) d_pos, stride_bytes, BoxSize, ctx->dd_tab.ptr, (unsigned long long *) d_keys);
        SHQ_HIP(hipGetLastError());
    }
    return SHQ_OK;
}

extern "C" int shq_domain_samples(shq_context *ctx, const shq_peano_tables *tables, const shq_domain_parts *parts, int SubSampleDistance, int PreSort,
                                  uint64_t *d_samples, int64_t *nsample)
{
    SHQ_CHECK(ctx && nsample && d_samples, SHQ_ERR_INVALID, "null argument");
    SHQ_TRY(check_parts(parts));
    SHQ_CHECK(SubSampleDistance >= 1, SHQ_ERR_INVALID, "domain_samples: SubSampleDistance must be positive");
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(use_tables(ctx, tables));
    hipStream_t st = ctx->stream;
    const long long np = parts->numpart, dist = SubSampleDistance;
    *nsample = 0;
    if(np == 0)
        return SHQ_OK;
    long long nkeys = np; /* PreSort: every slot */
    long long kdist = 1;
    if(!PreSort) {
        nkeys = np / dist;
        if(nkeys == 0)
            nkeys = 1;
        kdist = dist;
    }
    SHQ_TRY(ctx->dd_u64[0].reserve((size_t) nkeys));
    SHQ_TRY(ctx->dd_u64[1].reserve((size_t) nkeys));
    SHQ_TRY(ctx->dd_u64[2].reserve(2));
    SHQ_HIP(hipMemsetAsync(ctx->dd_u64[2].ptr, 0, sizeof(unsigned long long), st));
    dd_sample_keys_kernel<<<dim3(nblk(nkeys)), dim3(256), 0, st>>>(nkeys, kdist, (const char *) parts->d_parts, parts->elsize, parts->off_flags, parts->off_pos,
                                                                   parts->BoxSize, ctx->dd_tab.ptr, ctx->dd_u64[0].ptr, ctx->dd_u64[2].ptr);
    SHQ_HIP(hipGetLastError());
    /* garbage (PEANOCELLS) sorts behind every key */
    SHQ_TRY(prim_sort_keys(ctx, ctx->dd_u64[0].ptr, ctx->dd_u64[1].ptr, (size_t) nkeys, 0, 64));
    unsigned long long live = 0;
    SHQ_HIP(hipMemcpyAsync(&live, ctx->dd_u64[2].ptr, sizeof(live), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    long long ns;
    if(PreSort) {
        ns = (long long) live / dist;
        if(ns == 0 && live > 0)
            ns = 1;
        if(ns > 0) {
            dd_stride_kernel<<<dim3(nblk(ns)), dim3(256), 0, st>>>(ns, dist, ctx->dd_u64[1].ptr, (unsigned long long *) d_samples);
            SHQ_HIP(hipGetLastError());
        }
    } else {
        ns = (long long) live;
        if(ns > 0)
            SHQ_HIP(hipMemcpyAsync(d_samples, ctx->dd_u64[1].ptr, sizeof(uint64_t) * (size_t) ns, hipMemcpyDeviceToDevice, st));
    }
    *nsample = ns;
    return SHQ_OK;
}

extern "C" int shq_domain_local_toptree(shq_context *ctx, const uint64_t *d_sorted_samples, int64_t nsample, int64_t countlimit, int64_t costlimit, int MaxTopNodes,
                                        shq_local_topnode *tree, int *size)
{
    SHQ_CHECK(ctx && tree && size && (nsample == 0 || d_sorted_samples), SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(nsample >= 0 && nsample < (1ll << 31) - 64 && MaxTopNodes >= 1, SHQ_ERR_INVALID, "domain_local_toptree: bad sample count or MaxTopNodes");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const shq_local_topnode root = {0, 3 * SHQ_PEANO_BITS, -1, -1, 0, nsample, nsample};
    if(nsample < 2) { /* no pair, no split */
        tree[0] = root;
        *size = 1;
        return SHQ_OK;
    }
    const long long n = nsample;
    const unsigned long long *k = (const unsigned long long *) d_sorted_samples;
    SHQ_TRY(ctx->dd_i64[0].reserve((size_t) n + 1));
    SHQ_TRY(ctx->dd_i64[1].reserve((size_t) n + 1));
    long long *c = ctx->dd_i64[0].ptr, *S = ctx->dd_i64[1].ptr;
    dd_nsplit_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, k, c);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(prim_exclusive_scan(ctx, c, S, 0ll, (size_t) n));
    long long tail[2] = {0, 0};
    SHQ_HIP(hipMemcpyAsync(&tail[0], S + (n - 1), sizeof(long long), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipMemcpyAsync(&tail[1], c + (n - 1), sizeof(long long), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    const long long nnodes = 1 + 8 * (tail[0] + tail[1]);
    if(nnodes > MaxTopNodes) {
        shq_set_error("domain_local_toptree: the skeleton has %lld nodes, MaxTopNodes is %d: retry with more", nnodes, MaxTopNodes);
        return SHQ_ERR_RETRY;
    }
    SHQ_TRY(ctx->dd_u64[0].reserve((size_t) nnodes));
    SHQ_TRY(ctx->dd_i32[0].reserve((size_t) nnodes));
    SHQ_TRY(ctx->dd_i32[1].reserve((size_t) nnodes));
    SHQ_TRY(ctx->dd_i32[2].reserve((size_t) nnodes + 2));
    SHQ_TRY(ctx->dd_u8.reserve((size_t) nnodes));
    SHQ_TRY(ctx->dd_rec.reserve(sizeof(shq_local_topnode) * (size_t) nnodes + sizeof(int32_t) * (size_t) nnodes));
    DdSkel sk{ctx->dd_u64[0].ptr, ctx->dd_i32[0].ptr, ctx->dd_i32[1].ptr, ctx->dd_i32[2].ptr};
    SHQ_HIP(hipMemsetAsync(sk.Daughter, 0xff, sizeof(int32_t) * (size_t) nnodes, st));
    dd_split_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, k, S, sk, nnodes);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipStreamSynchronize(st));
    SHQ_TRY(ctx->dd_i64[0].reserve((size_t) std::max(n + 1, nnodes))); /* the split counts are used up; their buffer takes the node counts */
    long long *count = ctx->dd_i64[0].ptr;
    dd_count_kernel<<<dim3(nblk(nnodes)), dim3(256), 0, st>>>(nnodes, sk, k, n, count);
    SHQ_HIP(hipGetLastError());
    const long long lim = std::min<long long>(countlimit, costlimit);
    dd_flag_kernel<<<dim3(nblk(nnodes)), dim3(256), 0, st>>>(nnodes, sk, count, lim, ctx->dd_u8.ptr);
    SHQ_HIP(hipGetLastError());
    int32_t *list = reinterpret_cast<int32_t *>(ctx->dd_rec.ptr + sizeof(shq_local_topnode) * (size_t) nnodes);
    int64_t nkeep = 0;
    SHQ_TRY(prim_select_flagged(ctx, rocprim::counting_iterator<int32_t>(0), ctx->dd_u8.ptr, list, (size_t) nnodes, nullptr, &nkeep));
    SHQ_CHECK(nkeep >= 1 && nkeep <= nnodes && (nkeep - 1) % 8 == 0, SHQ_ERR_DEVICE, "domain_local_toptree: %lld survivors of %lld nodes", (long long) nkeep, nnodes);
    shq_local_topnode *d_out = reinterpret_cast<shq_local_topnode *>(ctx->dd_rec.ptr);
    dd_gather_kernel<<<dim3(nblk(nkeep)), dim3(256), 0, st>>>(nkeep, list, sk, count, lim, d_out);
    SHQ_HIP(hipGetLastError());
    std::vector<shq_local_topnode> nodes(nkeep);
    std::vector<int32_t> old(nkeep);
    SHQ_HIP(hipMemcpyAsync(nodes.data(), d_out, sizeof(shq_local_topnode) * nkeep, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipMemcpyAsync(old.data(), list, sizeof(int32_t) * nkeep, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    /* domain_toptree_garbage_collection's numbering of the survivors */
    dh::toptree_renumber(nodes, old, tree);
    *size = (int) nkeep;
    return SHQ_OK;
}

extern "C" int shq_domain_toptree_merge(shq_local_topnode *treeA, int *sizeA, const shq_local_topnode *treeB, int sizeB, int MaxTopNodes)
{
    SHQ_CHECK(treeA && sizeA && treeB && *sizeA >= 1 && sizeB >= 1 && *sizeA <= MaxTopNodes, SHQ_ERR_INVALID, "domain_toptree_merge: bad trees");
    const int rc = dh::toptree_merge_r(treeA, treeB, 0, 0, sizeA, sizeB, MaxTopNodes);
    if(rc == SHQ_ERR_RETRY)
        shq_set_error("domain_toptree_merge: no room for eight more nodes in %d", MaxTopNodes);
    else if(rc != SHQ_OK)
        shq_set_error("domain_toptree_merge: treeB is corrupt");
    return rc;
}

extern "C" int shq_domain_toptree_finish(shq_local_topnode *tree, int *size, int MaxTopNodes, int64_t countlimit, int64_t costlimit, shq_topnode *TopNodes,
                                         shq_topleaf *TopLeaves, int *ntopleaves)
{
    SHQ_CHECK(tree && size && TopNodes && TopLeaves && ntopleaves && *size >= 1 && *size <= MaxTopNodes, SHQ_ERR_INVALID, "domain_toptree_finish: bad arguments");
    const int rc = dh::global_refine(tree, size, MaxTopNodes, countlimit, costlimit);
    if(rc != SHQ_OK) {
        shq_set_error("domain_toptree_finish: global refine ran out of top nodes (%d)", MaxTopNodes);
        return rc;
    }
    for(int i = 0; i < *size; i++)
        TopNodes[i] = shq_topnode{tree[i].StartKey, tree[i].Daughter, tree[i].Shift, -1, 0};
    const int nl = dh::create_topleaves(TopNodes, *size, TopLeaves);
    SHQ_CHECK(nl >= 1, SHQ_ERR_INVALID, "domain_toptree_finish: a Daughter does not lie behind its node");
    *ntopleaves = nl;
    return SHQ_OK;
}

extern "C" int shq_domain_balance(shq_topnode *TopNodes, int ntopnodes, shq_topleaf *TopLeaves, int ntopleaves, const int64_t *TopLeafCount, int NTask,
                                  int64_t MaxPart, double SetAsideFactor, shq_task_leafs *Tasks, int *status)
{
    SHQ_CHECK(TopNodes && TopLeaves && TopLeafCount && Tasks && status && NTask >= 1 && ntopnodes >= 1, SHQ_ERR_INVALID, "domain_balance: bad arguments");
    SHQ_CHECK(ntopleaves >= NTask, SHQ_ERR_INVALID, "domain_balance: Number of Topleaves is less than NTask");
    for(int i = 0; i < ntopleaves; i++)
        SHQ_CHECK(TopLeaves[i].topnode >= 0 && TopLeaves[i].topnode < ntopnodes && TopLeafCount[i] >= 0, SHQ_ERR_INVALID, "domain_balance: leaf %d names no top node", i);
    SHQ_CHECK(dh::assign_topleaves_balanced(TopNodes, TopLeaves, ntopleaves, TopLeafCount, NTask) == SHQ_OK, SHQ_ERR_INVALID,
              "domain_balance: not enough segments were created, or cost left unassigned");
    SHQ_CHECK(dh::set_task_leafs(TopLeaves, ntopleaves, NTask, Tasks) == SHQ_OK, SHQ_ERR_INVALID, "domain_balance: the leaves do not name %d tasks in order", NTask);
    *status = dh::check_memory_bound(Tasks, NTask, TopLeafCount, MaxPart, SetAsideFactor);
    return SHQ_OK;
}

extern "C" int shq_domain_install(shq_context *ctx, const shq_peano_tables *tables, const shq_topnode *TopNodes, int ntopnodes, const shq_topleaf *TopLeaves,
                                  int ntopleaves, shq_topnode_geo *geo_out)
{
    SHQ_CHECK(ctx && TopNodes && TopLeaves && ntopnodes >= 1 && ntopleaves >= 1, SHQ_ERR_INVALID, "domain_install: bad arguments");
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(use_tables(ctx, tables));
    std::vector<uint8_t> state((size_t) ntopnodes, 0);
    std::vector<DdNode> nodes((size_t) ntopnodes);
    for(int t = 0; t < ntopnodes; t++) {
        const shq_topnode &nd = TopNodes[t];
        nodes[t] = DdNode{nd.StartKey, nd.Daughter, nd.Shift, nd.Leaf, 0};
        if(nd.Daughter < 0) {
            SHQ_CHECK(nd.Leaf >= 0 && nd.Leaf < ntopleaves, SHQ_ERR_INVALID, "domain_install: top node %d is a leaf without a TopLeaves entry", t);
            nodes[t].Daughter = -1;
        } else
            SHQ_CHECK(nd.Daughter > t && nd.Daughter + 8 <= ntopnodes && nd.Shift >= 3 && nd.Shift <= 3 * SHQ_PEANO_BITS, SHQ_ERR_INVALID,
                      "domain_install: top node %d: Daughter %d / Shift %d describe no tree", t, nd.Daughter, nd.Shift);
        if(geo_out) {
            for(int o = 0; o < 8; o++)
                geo_out[t].daughter[o] = -1;
            geo_out[t].leaf = nd.Daughter < 0 ? nd.Leaf : -1;
            geo_out[t].pad_ = 0;
        }
        if(nd.Daughter >= 0)
            for(int i = 0; i < 2; i++)
                for(int j = 0; j < 2; j++)
                    for(int k = 0; k < 2; k++) {
                        const int o = (i << 2) | (j << 1) | k, d = nd.Daughter + tables->sub[state[t]][o];
                        state[d] = tables->next[state[t]][o];
                        if(geo_out)
                            geo_out[t].daughter[i + 2 * j + 4 * k] = d;
                    }
    }
    std::vector<int32_t> task((size_t) ntopleaves);
    for(int l = 0; l < ntopleaves; l++)
        task[l] = TopLeaves[l].Task;
    ctx->dd_ntopnodes = ctx->dd_ntopleaves = 0;
    SHQ_TRY(ctx->dd_nodes.reserve(sizeof(DdNode) * (size_t) ntopnodes));
    SHQ_TRY(ctx->dd_leaf_task.reserve((size_t) ntopleaves));
    SHQ_HIP(hipMemcpyAsync(ctx->dd_nodes.ptr, nodes.data(), sizeof(DdNode) * (size_t) ntopnodes, hipMemcpyHostToDevice, ctx->stream));
    SHQ_HIP(hipMemcpyAsync(ctx->dd_leaf_task.ptr, task.data(), sizeof(int32_t) * (size_t) ntopleaves, hipMemcpyHostToDevice, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* the staging vectors live on this frame */
    ctx->dd_ntopnodes = ntopnodes;
    ctx->dd_ntopleaves = ntopleaves;
    return SHQ_OK;
}

extern "C" int shq_domain_leaf_counts(shq_context *ctx, const shq_domain_parts *parts, int64_t *TopLeafCount)
{
    SHQ_CHECK(ctx && TopLeafCount, SHQ_ERR_INVALID, "null argument");
    SHQ_TRY(check_parts(parts));
    SHQ_CHECK(ctx->dd_ntopnodes > 0 && ctx->dd_tab_valid, SHQ_ERR_STATE, "domain_leaf_counts: needs shq_domain_install");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int nl = ctx->dd_ntopleaves;
    const long long n = parts->numpart;
    SHQ_TRY(ctx->dd_u64[0].reserve((size_t) nl));
    SHQ_HIP(hipMemsetAsync(ctx->dd_u64[0].ptr, 0, sizeof(unsigned long long) * (size_t) nl, st));
    if(n > 0) {
        const DdNode *nodes = reinterpret_cast<const DdNode *>(ctx->dd_nodes.ptr);
        if(nl <= DD_LDS_BINS) {
            const unsigned blocks = std::min(nblk(n), 2048u); /* 8 workgroups per compute unit; each folds its bins once */
            dd_leafcount_lds_kernel<<<dim3(blocks), dim3(256), 0, st>>>(n, (const char *) parts->d_parts, parts->elsize, parts->off_flags, parts->off_pos, parts->BoxSize,
                                                                        ctx->dd_tab.ptr, nodes, nl, ctx->dd_u64[0].ptr);
        } else
            dd_leafcount_global_kernel<<<dim3(nblk(n)), dim3(256), 0, st>>>(n, (const char *) parts->d_parts, parts->elsize, parts->off_flags, parts->off_pos,
                                                                           parts->BoxSize, ctx->dd_tab.ptr, nodes, nl, ctx->dd_u64[0].ptr);
        SHQ_HIP(hipGetLastError());
    }
    SHQ_HIP(hipMemcpyAsync(TopLeafCount, ctx->dd_u64[0].ptr, sizeof(int64_t) * (size_t) nl, hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    return SHQ_OK;
}

extern "C" int shq_domain_particle_topleaves(shq_context *ctx, const shq_domain_parts *parts, int32_t *d_topleaf, int32_t *d_target)
{
    SHQ_CHECK(ctx && (d_topleaf || (parts && parts->numpart == 0)), SHQ_ERR_INVALID, "null argument");
    SHQ_TRY(check_parts(parts));
    SHQ_CHECK(ctx->dd_ntopnodes > 0 && ctx->dd_tab_valid, SHQ_ERR_STATE, "domain_particle_topleaves: needs shq_domain_install");
    SHQ_HIP(hipSetDevice(ctx->device));
    const long long n = parts->numpart;
    if(n > 0) {
        dd_particle_leaf_kernel<<<dim3(nblk(n)), dim3(256), 0, ctx->stream>>>(n, (const char *) parts->d_parts, parts->elsize, parts->off_flags, parts->off_pos,
                                                                             parts->BoxSize, ctx->dd_tab.ptr, reinterpret_cast<const DdNode *>(ctx->dd_nodes.ptr),
                                                                             ctx->dd_leaf_task.ptr, ctx->dd_ntopleaves, d_topleaf, d_target);
        SHQ_HIP(hipGetLastError());
    }
    return SHQ_OK;
}
