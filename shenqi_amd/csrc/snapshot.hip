/* snapshot.hip — the per-particle loops of a snapshot on device-resident records (include/shenqi_hip.h, "Snapshot blocks").
 *
 *   petaio_build_selection   petaio.cpp:86-128 (fof_select_func, fofpetaio.cpp:33-36)     shq_io_select
 *   petaio_build_buffer      petaio.cpp:550-575 with the getters :673-894, :1012-1023      shq_io_gather
 *   petaio_readout_buffer    petaio.cpp:536-545 with the setters :684-893                  shq_io_scatter
 *
 * The gather.  A workgroup owns IO_TILE consecutive rows of the selection.  It stages their base records into LDS with 16-byte loads,
 * consecutive lanes on consecutive 16-byte pieces of consecutive records (a near-contiguous selection reads as a stream; the per-lane
 * source address makes the same loop a row gather), then lane k picks the fields of record k for every block that reads the base record
 * and writes row k of each column.  If a block reads the slot, the tile is then filled again with the slot records PI names, by the same
 * loop, and the slot blocks are picked by the same function.  So a record leaves HBM once per call, however many blocks read it.
 * The LDS row pitch is the record size rounded up to an odd number of 8-byte words (160 -> 168, 176 -> 184, 72, 248): 32 lanes reading
 * the same 8-byte member of 32 consecutive rows then touch all 64 banks once (DESIGN.md has the arithmetic).
 * The descriptors are kernel arguments: wave-uniform, read through scalar loads, every switch over them is a scalar branch. */
#include "device_prims.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int IO_TILE = 128;
constexpr size_t IO_MAXREC = 480; /* IO_TILE * (480 + 8) bytes of LDS stay below the 64 KiB a launch gets without asking */
enum { IO_E_INDEX = 1, IO_E_TYPE = 2, IO_E_PI = 4, IO_E_POSITION = 8 };
enum { IO_KEY_NONE = 6, IO_KEY_BAD = 7 };

struct IoBlocks {
    shq_io_block b[SHQ_IO_MAXBLOCKS];
    char *col[SHQ_IO_MAXBLOCKS];
    int n;
};
struct IoRec { /* how to find a particle's members */
    const char *parts;
    size_t elsize, off_flags, off_type, off_pi, off_grnr;
    long long numpart;
};

/* a value on its way from one C type to another: a double, a signed or an unsigned 64-bit integer */
struct IoVal {
    int cls; /* 0 double, 1 signed, 2 unsigned */
    double d;
    unsigned long long u;
};

__host__ __device__ inline int io_size(int t)
{
    switch(t) {
        case SHQ_IO_F64: case SHQ_IO_I64: case SHQ_IO_U64: return 8;
        case SHQ_IO_F32: case SHQ_IO_I32: case SHQ_IO_U32: return 4;
        default: return 1;
    }
}
inline size_t io_pitch(size_t elsize) { return ((elsize / 8) & 1) ? elsize : elsize + 8; }

__device__ __forceinline__ IoVal io_load(const char *p, int t, int shift, int width)
{
    IoVal v{2, 0.0, 0ull};
    switch(t) {
        case SHQ_IO_F64: v.cls = 0; v.d = *reinterpret_cast<const double *>(p); break;
        case SHQ_IO_F32: v.cls = 0; v.d = (double) *reinterpret_cast<const float *>(p); break;
        case SHQ_IO_I64: v.cls = 1; v.u = (unsigned long long) *reinterpret_cast<const long long *>(p); break;
        case SHQ_IO_U64: v.u = *reinterpret_cast<const unsigned long long *>(p); break;
        case SHQ_IO_I32: v.cls = 1; v.u = (unsigned long long) (long long) *reinterpret_cast<const int32_t *>(p); break;
        case SHQ_IO_U32: v.u = *reinterpret_cast<const uint32_t *>(p); break;
        case SHQ_IO_I8: v.cls = 1; v.u = (unsigned long long) (long long) *reinterpret_cast<const int8_t *>(p); break;
        case SHQ_IO_U8: v.u = *reinterpret_cast<const uint8_t *>(p); break;
        default: v.u = (*reinterpret_cast<const uint8_t *>(p) >> shift) & ((1u << width) - 1u); break;
    }
    return v;
}

template <typename T> __device__ __forceinline__ T io_as_int(const IoVal &v)
{
    if(v.cls == 0)
        return (T) v.d;
    return (T) v.u; /* wraps, as the C conversion between integer types does */
}

/* the C conversion to type t, stored at p; SHQ_IO_BITS replaces only its bits */
__device__ __forceinline__ void io_store(char *p, int t, int shift, int width, const IoVal &v)
{
    switch(t) {
        case SHQ_IO_F64: *reinterpret_cast<double *>(p) = v.cls == 0 ? v.d : v.cls == 1 ? (double) (long long) v.u : (double) v.u; break;
        case SHQ_IO_F32: *reinterpret_cast<float *>(p) = v.cls == 0 ? (float) v.d : v.cls == 1 ? (float) (long long) v.u : (float) v.u; break;
        case SHQ_IO_I64: *reinterpret_cast<long long *>(p) = io_as_int<long long>(v); break;
        case SHQ_IO_U64: *reinterpret_cast<unsigned long long *>(p) = io_as_int<unsigned long long>(v); break;
        case SHQ_IO_I32: *reinterpret_cast<int32_t *>(p) = io_as_int<int32_t>(v); break;
        case SHQ_IO_U32: *reinterpret_cast<uint32_t *>(p) = io_as_int<uint32_t>(v); break;
        case SHQ_IO_I8: *reinterpret_cast<int8_t *>(p) = io_as_int<int8_t>(v); break;
        case SHQ_IO_U8: *reinterpret_cast<uint8_t *>(p) = io_as_int<uint8_t>(v); break;
        default: {
            const unsigned m = ((1u << width) - 1u) << shift;
            uint8_t *q = reinterpret_cast<uint8_t *>(p);
            *q = (uint8_t) ((*q & ~m) | ((io_as_int<unsigned>(v) << shift) & m));
        }
    }
}

/* GAMMA_MINUS1 as the reference forms it: (5.0 / 3.0) - 1, which is not 2.0 / 3.0 */
#define IO_GAMMA_MINUS1 ((5.0 / 3.0) - 1)

/* one getter: the members of record `rec` (in LDS) that block b names, into row `row` of its column */
__device__ __forceinline__ void io_get(const shq_io_block &b, const char *rec, char *col, long long row, const shq_io_conv &cv, int *err)
{
#pragma clang fp contract(off)
    const int fs = io_size(b.field_type), cs = io_size(b.col_type);
    char *out = col + (size_t) row * (size_t) b.items * (size_t) cs;
    if(b.kind == SHQ_IO_INTERNAL_ENERGY) {
        const double Entropy = *reinterpret_cast<const double *>(rec + b.offset), Density = *reinterpret_cast<const double *>(rec + b.offset2);
        const double a3inv = 1 / (cv.atime * cv.atime * cv.atime);
        const IoVal v{0, Entropy / IO_GAMMA_MINUS1 * pow(Density * a3inv, IO_GAMMA_MINUS1), 0ull};
        io_store(out, b.col_type, 0, 0, v);
        return;
    }
    for(int k = 0; k < b.items; k++) {
        IoVal v = io_load(rec + b.offset + (size_t) k * fs, b.field_type, b.bit_shift, b.bit_width);
        if(b.kind == SHQ_IO_POSITION) {
            double o = v.d - cv.CurrentParticleOffset[k % 3];
            if(!isfinite(o)) {
                atomicOr(err, IO_E_POSITION);
                continue;
            }
            int r;
            for(r = 0; r < 64 && o > cv.BoxSize; r++)
                o -= cv.BoxSize;
            if(o > cv.BoxSize)
                atomicOr(err, IO_E_POSITION);
            for(r = 0; r < 64 && o <= 0; r++)
                o += cv.BoxSize;
            if(o <= 0)
                atomicOr(err, IO_E_POSITION);
            v.d = o;
        } else if(b.kind == SHQ_IO_SCALE)
            v.d = cv.fac * v.d;
        io_store(out + (size_t) k * cs, b.col_type, 0, 0, v);
    }
}

/* one setter: row `row` of the column into the members of the record at `rec` (global memory) */
__device__ __forceinline__ void io_set(const shq_io_block &b, char *rec, const char *col, long long row, const shq_io_conv &cv)
{
#pragma clang fp contract(off)
    const int fs = io_size(b.field_type), cs = io_size(b.col_type);
    const char *in = col + (size_t) row * (size_t) b.items * (size_t) cs;
    if(b.kind == SHQ_IO_INTERNAL_ENERGY) {
        const double u = io_load(in, b.col_type, 0, 0).d;
        const double Density = *reinterpret_cast<const double *>(rec + b.offset2);
        const double a3inv = 1 / (cv.atime * cv.atime * cv.atime);
        *reinterpret_cast<double *>(rec + b.offset) = IO_GAMMA_MINUS1 * u / pow(Density * a3inv, IO_GAMMA_MINUS1);
        return;
    }
    for(int k = 0; k < b.items; k++) {
        IoVal v = io_load(in + (size_t) k * cs, b.col_type, 0, 0);
        if(b.kind == SHQ_IO_SCALE)
            v.d = v.d * cv.fac;
        io_store(rec + b.offset + (size_t) k * fs, b.field_type, b.bit_shift, b.bit_width, v);
    }
}

/* records s_src[0 .. nrow) of an array of R-byte records into the tile, CH bytes per lane and step.  IO_BATCH loads are issued before
 * the first of them is stored, so that a lane has IO_BATCH * 16 bytes in flight (about 70 KiB per compute unit at the occupancy the tile
 * allows), which is what hides the latency of HBM; one load per trip of the loop does not.  The loads are unconditional so that the
 * compiler can batch them: a row with s_src < 0 (refused by a check) reads `dummy`, 16 valid bytes, and is never picked. */
constexpr int IO_BATCH = 5;
template <int CH>
__device__ __forceinline__ void io_stage(char *lds, unsigned pitch, const char *__restrict__ base, unsigned R, const int *s_src, int nrow, const char *__restrict__ dummy)
{
    const unsigned P = R / CH, total = (unsigned) nrow * P;
    for(unsigned t0 = threadIdx.x; t0 < total; t0 += IO_TILE * IO_BATCH) {
        uint4 v[IO_BATCH];
        unsigned dst[IO_BATCH];
#pragma unroll
        for(int u = 0; u < IO_BATCH; u++) {
            const unsigned t = t0 + (unsigned) u * IO_TILE;
            const unsigned rec = t / P, piece = t - rec * P;
            const int src = t < total ? s_src[rec] : -1;
            const char *g = src >= 0 ? base + (size_t) src * R + (size_t) piece * CH : dummy;
            dst[u] = t < total ? rec * pitch + piece * CH : ~0u;
            if(CH == 16)
                v[u] = *reinterpret_cast<const uint4 *>(g);
            else {
                const uint2 w = *reinterpret_cast<const uint2 *>(g);
                v[u] = make_uint4(w.x, w.y, 0u, 0u);
            }
        }
#pragma unroll
        for(int u = 0; u < IO_BATCH; u++)
            if(dst[u] != ~0u) {
                uint2 *l = reinterpret_cast<uint2 *>(lds + dst[u]); /* two 8-byte stores: the pitch keeps 8-byte alignment only */
                l[0] = make_uint2(v[u].x, v[u].y);
                if(CH == 16)
                    l[1] = make_uint2(v[u].z, v[u].w);
            }
    }
}

__global__ __launch_bounds__(IO_TILE) void io_gather_kernel(IoRec pr, const char *__restrict__ slots, unsigned slot_elsize, long long slot_size, int ptype,
                                                            const int32_t *__restrict__ sel, long long n, IoBlocks B, shq_io_conv cv, int need_slot, unsigned pitch_base,
                                                            unsigned pitch_slot, int wide_base, int wide_slot, int *err, const char *__restrict__ dummy)
{
    extern __shared__ uint2 io_tile_[];
    __shared__ int s_src[IO_TILE];
    char *lds = reinterpret_cast<char *>(io_tile_);
    const long long row0 = (long long) blockIdx.x * IO_TILE;
    const int nrow = (int) (n - row0 < IO_TILE ? n - row0 : IO_TILE);
    const int k = threadIdx.x;
    const long long row = row0 + k;
    bool ok = k < nrow;
    if(ok) {
        const int idx = sel[row];
        if(idx < 0 || idx >= pr.numpart) { /* before the record is read */
            atomicOr(err, IO_E_INDEX);
            ok = false;
        }
        s_src[k] = ok ? idx : -1;
    } else
        s_src[k] = -1;
    __syncthreads();
    if(wide_base)
        io_stage<16>(lds, pitch_base, pr.parts, (unsigned) pr.elsize, s_src, nrow, dummy);
    else
        io_stage<8>(lds, pitch_base, pr.parts, (unsigned) pr.elsize, s_src, nrow, dummy);
    __syncthreads();
    int pi = -1;
    if(ok) {
        const char *rec = lds + (unsigned) k * pitch_base;
        if(*reinterpret_cast<const uint8_t *>(rec + pr.off_type) != ptype) { /* "Selection %d has type = %d != %d" */
            atomicOr(err, IO_E_TYPE);
            ok = false;
        } else {
            pi = *reinterpret_cast<const int32_t *>(rec + pr.off_pi);
            for(int b = 0; b < B.n; b++)
                if(B.b[b].source == SHQ_IO_SRC_BASE)
                    io_get(B.b[b], rec, B.col[b], row, cv, err);
        }
    }
    if(!need_slot) /* uniform */
        return;
    if(ok && (pi < 0 || pi >= slot_size)) { /* before the slot is read */
        atomicOr(err, IO_E_PI);
        ok = false;
    }
    __syncthreads(); /* every lane is done with the base records */
    s_src[k] = ok ? pi : -1;
    __syncthreads();
    if(wide_slot)
        io_stage<16>(lds, pitch_slot, slots, slot_elsize, s_src, nrow, dummy);
    else
        io_stage<8>(lds, pitch_slot, slots, slot_elsize, s_src, nrow, dummy);
    __syncthreads();
    if(ok) {
        const char *rec = lds + (unsigned) k * pitch_slot;
        for(int b = 0; b < B.n; b++)
            if(B.b[b].source == SHQ_IO_SRC_SLOT)
                io_get(B.b[b], rec, B.col[b], row, cv, err);
    }
}

/* the readout's check: every particle of the list has its slot inside the array */
__global__ void io_scatter_check_kernel(IoRec pr, const int32_t *__restrict__ list, long long cnt, long long slot_size, int *err)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= cnt)
        return;
    const int pi = *reinterpret_cast<const int32_t *>(pr.parts + (size_t) list[k] * pr.elsize + pr.off_pi);
    if(pi < 0 || pi >= slot_size)
        atomicOr(err, IO_E_PI);
}

/* row k to the k-th particle of the type: one lane per particle, its blocks in array order */
__global__ __launch_bounds__(256) void io_scatter_kernel(IoRec pr, char *parts, char *slots, size_t slot_elsize, const int32_t *__restrict__ list, long long cnt,
                                                         IoBlocks B, shq_io_conv cv)
{
    const long long k = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(k >= cnt)
        return;
    char *rec = parts + (size_t) list[k] * pr.elsize;
    for(int b = 0; b < B.n; b++) {
        char *dst = rec;
        if(B.b[b].source == SHQ_IO_SRC_SLOT) /* PI as it is now: no block writes it, and the check has seen it */
            dst = slots + (size_t) *reinterpret_cast<const int32_t *>(rec + pr.off_pi) * slot_elsize;
        io_set(B.b[b], dst, B.col[b], k, cv);
    }
}

__global__ void io_typeflag_kernel(IoRec pr, int ptype, uint8_t *__restrict__ flag)
{
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(i < pr.numpart)
        flag[i] = *reinterpret_cast<const uint8_t *>(pr.parts + (size_t) i * pr.elsize + pr.off_type) == ptype;
}

/* the type key of every particle (its Type, IO_KEY_NONE when it is not selected, IO_KEY_BAD for a selected Type > 5), the counts by key,
 * and under SHQ_IO_ORDER_GRNR the GrNr with its sign bit flipped, which orders as the signed value does */
__global__ __launch_bounds__(256) void io_keys_kernel(IoRec pr, int predicate, uint8_t *__restrict__ key, unsigned long long *__restrict__ grnr,
                                                      unsigned long long *__restrict__ counts)
{
    __shared__ unsigned int bins[8];
    if(threadIdx.x < 8)
        bins[threadIdx.x] = 0;
    __syncthreads();
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    int kk = -1;
    if(i < pr.numpart) {
        const char *p = pr.parts + (size_t) i * pr.elsize;
        const uint8_t fl = *reinterpret_cast<const uint8_t *>(p + pr.off_flags);
        bool take = !(fl & 1u);
        long long g = 0;
        if(predicate == SHQ_IO_SELECT_FOF || grnr)
            g = *reinterpret_cast<const long long *>(p + pr.off_grnr);
        if(predicate == SHQ_IO_SELECT_FOF)
            take = take && g >= 0 && !(fl & 2u);
        kk = IO_KEY_NONE;
        if(take) {
            const int type = *reinterpret_cast<const uint8_t *>(p + pr.off_type);
            kk = type > 5 ? IO_KEY_BAD : type;
        }
        key[i] = (uint8_t) kk;
        if(grnr)
            grnr[i] = (unsigned long long) g ^ (1ull << 63);
    }
    for(int v = 0; v < 8; v++) { /* one add per wave and key, not one per particle on the same few bins */
        const unsigned long long m = shq_ballot(kk == v);
        if((threadIdx.x & 63) == 0 && m)
            atomicAdd(&bins[v], (unsigned int) __popcll((long long) m));
    }
    __syncthreads();
    if(threadIdx.x < 8 && bins[threadIdx.x])
        atomicAdd(&counts[threadIdx.x], (unsigned long long) bins[threadIdx.x]);
}

__global__ void io_key_of_kernel(long long n, const int32_t *__restrict__ idx, const uint8_t *__restrict__ key, uint8_t *__restrict__ out)
{
    const long long j = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if(j < n)
        out[j] = key[idx[j]];
}

int check_layout(const shq_io_layout *l, const void *d_parts, int64_t numpart, bool need_grnr)
{
    SHQ_CHECK(l && numpart >= 0 && numpart < (1ll << 31) - 64 && (d_parts || numpart == 0), SHQ_ERR_INVALID, "snapshot: bad particle array");
    SHQ_CHECK(l->part_elsize >= 8 && l->part_elsize % 8 == 0 && l->part_elsize <= IO_MAXREC && ((uintptr_t) d_parts % 8) == 0, SHQ_ERR_INVALID,
              "snapshot: records are 8-byte aligned, a multiple of 8 and at most %zu bytes", IO_MAXREC);
    SHQ_CHECK(l->off_flags < l->part_elsize && l->off_type < l->part_elsize && l->off_pi % 4 == 0 && l->off_pi + 4 <= l->part_elsize, SHQ_ERR_INVALID,
              "snapshot: the flag byte, Type and PI must lie inside the record");
    SHQ_CHECK(!need_grnr || (l->off_grnr % 8 == 0 && l->off_grnr + 8 <= l->part_elsize), SHQ_ERR_INVALID, "snapshot: GrNr must be an aligned int64 inside the record");
    return SHQ_OK;
}

bool col_type_ok(int t) { return t >= SHQ_IO_F64 && t <= SHQ_IO_U8; }

/* every member a block names lies inside its record, aligned to its own size */
int check_blocks(const shq_io_layout *l, int ptype, const shq_io_block *blocks, int nblocks, const void *const *cols, int64_t n, bool *need_slot)
{
    SHQ_CHECK(nblocks >= 0 && (nblocks == 0 || (blocks && cols)), SHQ_ERR_INVALID, "snapshot: null block array");
    *need_slot = false;
    for(int b = 0; b < nblocks; b++) {
        const shq_io_block &k = blocks[b];
        SHQ_CHECK(k.source == SHQ_IO_SRC_BASE || k.source == SHQ_IO_SRC_SLOT, SHQ_ERR_INVALID, "snapshot: block %d: source %d", b, k.source);
        SHQ_CHECK(k.kind >= SHQ_IO_COPY && k.kind <= SHQ_IO_INTERNAL_ENERGY, SHQ_ERR_INVALID, "snapshot: block %d: kind %d", b, k.kind);
        SHQ_CHECK(k.field_type >= SHQ_IO_F64 && k.field_type <= SHQ_IO_BITS && col_type_ok(k.col_type), SHQ_ERR_INVALID, "snapshot: block %d: element types %d -> %d", b,
                  k.field_type, k.col_type);
        SHQ_CHECK(k.items >= 1 && k.items <= 64, SHQ_ERR_INVALID, "snapshot: block %d: %d items", b, k.items);
        const size_t rec = k.source == SHQ_IO_SRC_BASE ? l->part_elsize : l->slot_elsize[ptype];
        SHQ_CHECK(rec > 0, SHQ_ERR_INVALID, "snapshot: block %d reads the slot of type %d, which has none", b, ptype);
        const size_t fs = (size_t) io_size(k.field_type);
        SHQ_CHECK(k.offset % fs == 0 && k.offset + fs * (size_t) k.items <= rec, SHQ_ERR_INVALID, "snapshot: block %d: %d members at offset %llu leave the %zu-byte record",
                  b, k.items, (unsigned long long) k.offset, rec);
        if(k.field_type == SHQ_IO_BITS)
            SHQ_CHECK(k.bit_shift >= 0 && k.bit_width >= 1 && k.bit_shift + k.bit_width <= 8 && k.kind == SHQ_IO_COPY, SHQ_ERR_INVALID, "snapshot: block %d: bit field %d+%d",
                      b, k.bit_shift, k.bit_width);
        if(k.kind == SHQ_IO_POSITION || k.kind == SHQ_IO_SCALE)
            SHQ_CHECK(k.field_type == SHQ_IO_F64 || k.field_type == SHQ_IO_F32, SHQ_ERR_INVALID, "snapshot: block %d: POSITION and SCALE read floating-point members", b);
        if(k.kind == SHQ_IO_POSITION)
            SHQ_CHECK(k.items <= 3, SHQ_ERR_INVALID, "snapshot: block %d: POSITION has at most 3 items", b);
        if(k.kind == SHQ_IO_INTERNAL_ENERGY)
            SHQ_CHECK(k.field_type == SHQ_IO_F64 && k.items == 1 && k.offset2 % 8 == 0 && k.offset2 + 8 <= rec, SHQ_ERR_INVALID,
                      "snapshot: block %d: INTERNAL_ENERGY reads two doubles, Entropy and Density", b);
        SHQ_CHECK(cols[b] || n == 0, SHQ_ERR_INVALID, "snapshot: block %d has no column", b);
        SHQ_CHECK(((uintptr_t) cols[b] % (size_t) io_size(k.col_type)) == 0, SHQ_ERR_INVALID, "snapshot: block %d: misaligned column", b);
        if(k.source == SHQ_IO_SRC_SLOT)
            *need_slot = true;
    }
    return SHQ_OK;
}

int check_slots(const shq_io_layout *l, int ptype, const void *const d_slots[6], const int64_t slot_size[6])
{
    SHQ_CHECK(d_slots && slot_size, SHQ_ERR_INVALID, "snapshot: a block names the slot but no slot arrays were given");
    const size_t es = l->slot_elsize[ptype];
    SHQ_CHECK(es >= 8 && es % 8 == 0 && es <= IO_MAXREC && slot_size[ptype] >= 0 && slot_size[ptype] < (1ll << 31) && (d_slots[ptype] || slot_size[ptype] == 0) &&
                  ((uintptr_t) d_slots[ptype] % 8) == 0,
              SHQ_ERR_INVALID, "snapshot: slot records of type %d are 8-byte aligned, a multiple of 8 and at most %zu bytes", ptype, IO_MAXREC);
    return SHQ_OK;
}

int check_conv(const shq_io_conv *cv, const shq_io_block *blocks, int nblocks, bool getter)
{
    for(int b = 0; b < nblocks; b++) {
        SHQ_CHECK(cv, SHQ_ERR_INVALID, "snapshot: null conversions");
        if(blocks[b].kind == SHQ_IO_POSITION && getter)
            SHQ_CHECK(cv->BoxSize > 0 && cv->BoxSize < 1e300 && std::isfinite(cv->CurrentParticleOffset[0]) && std::isfinite(cv->CurrentParticleOffset[1]) &&
                          std::isfinite(cv->CurrentParticleOffset[2]),
                      SHQ_ERR_INVALID, "snapshot: POSITION needs a finite positive BoxSize and finite offsets");
        if(blocks[b].kind == SHQ_IO_INTERNAL_ENERGY)
            SHQ_CHECK(cv->atime > 0 && std::isfinite(cv->atime), SHQ_ERR_INVALID, "snapshot: INTERNAL_ENERGY needs atime > 0");
        if(blocks[b].kind == SHQ_IO_SCALE)
            SHQ_CHECK(std::isfinite(cv->fac), SHQ_ERR_INVALID, "snapshot: SCALE needs a finite fac");
    }
    return SHQ_OK;
}

IoRec io_rec(const shq_io_layout *l, const void *d_parts, int64_t numpart)
{
    return IoRec{(const char *) d_parts, l->part_elsize, l->off_flags, l->off_type, l->off_pi, l->off_grnr, (long long) numpart};
}

int *io_err(shq_context *ctx) { return reinterpret_cast<int *>(ctx->io_cnt.ptr + 8); }

int io_reset(shq_context *ctx)
{
    SHQ_TRY(ctx->io_cnt.reserve(10));
    SHQ_HIP(hipMemsetAsync(ctx->io_cnt.ptr, 0, sizeof(unsigned long long) * 10, ctx->stream));
    return SHQ_OK;
}

} // namespace

extern "C" int shq_io_select(shq_context *ctx, const shq_io_layout *layout, const void *d_parts, int64_t numpart, int predicate, int order, int32_t *d_selection,
                             int64_t count[6], int64_t offset[6])
{
    SHQ_CHECK(ctx && count && offset, SHQ_ERR_INVALID, "null argument");
    SHQ_CHECK(predicate == SHQ_IO_SELECT_ALL || predicate == SHQ_IO_SELECT_FOF, SHQ_ERR_INVALID, "io_select: predicate %d", predicate);
    SHQ_CHECK(order == SHQ_IO_ORDER_INDEX || order == SHQ_IO_ORDER_GRNR, SHQ_ERR_INVALID, "io_select: order %d", order);
    const bool bygr = order == SHQ_IO_ORDER_GRNR;
    SHQ_TRY(check_layout(layout, d_parts, numpart, bygr || predicate == SHQ_IO_SELECT_FOF));
    SHQ_CHECK(d_selection || numpart == 0, SHQ_ERR_INVALID, "io_select: no selection array");
    for(int t = 0; t < 6; t++)
        count[t] = offset[t] = 0;
    if(numpart == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t N = (size_t) numpart;
    SHQ_TRY(io_reset(ctx));
    SHQ_TRY(ctx->io_u8[0].reserve(N));
    SHQ_TRY(ctx->io_u8[1].reserve(N));
    if(bygr) {
        SHQ_TRY(ctx->io_u64[0].reserve(N));
        SHQ_TRY(ctx->io_u64[1].reserve(N));
        SHQ_TRY(ctx->io_i32.reserve(N));
    }
    const IoRec pr = io_rec(layout, d_parts, numpart);
    io_keys_kernel<<<dim3(nblk(numpart)), dim3(256), 0, st>>>(pr, predicate, ctx->io_u8[0].ptr, bygr ? ctx->io_u64[0].ptr : nullptr, ctx->io_cnt.ptr);
    SHQ_HIP(hipGetLastError());
    if(!bygr)
        SHQ_TRY(prim_sort_pairs(ctx, ctx->io_u8[0].ptr, ctx->io_u8[1].ptr, rocprim::counting_iterator<int32_t>(0), d_selection, N, 0, 3));
    else {
        /* by GrNr first, then stably by type: within a type the order of GrNr, ties in index order */
        SHQ_TRY(prim_sort_pairs(ctx, ctx->io_u64[0].ptr, ctx->io_u64[1].ptr, rocprim::counting_iterator<int32_t>(0), ctx->io_i32.ptr, N, 0, 64));
        io_key_of_kernel<<<dim3(nblk(numpart)), dim3(256), 0, st>>>(numpart, ctx->io_i32.ptr, ctx->io_u8[0].ptr, ctx->io_u8[1].ptr);
        SHQ_HIP(hipGetLastError());
        SHQ_TRY(prim_sort_pairs(ctx, ctx->io_u8[1].ptr, ctx->io_u8[0].ptr, ctx->io_i32.ptr, d_selection, N, 0, 3));
    }
    unsigned long long h[8];
    SHQ_HIP(hipMemcpyAsync(h, ctx->io_cnt.ptr, sizeof(h), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    SHQ_CHECK(h[IO_KEY_BAD] == 0, SHQ_ERR_INVALID, "io_select: %llu selected particles with Type > 5", h[IO_KEY_BAD]);
    for(int t = 0; t < 6; t++) {
        count[t] = (int64_t) h[t];
        offset[t] = t ? offset[t - 1] + count[t - 1] : 0;
    }
    return SHQ_OK;
}

extern "C" int shq_io_gather(shq_context *ctx, const shq_io_layout *layout, const void *d_parts, int64_t numpart, const void *const d_slots[6],
                             const int64_t slot_size[6], int ptype, const int32_t *d_selection, int64_t n, const shq_io_block *blocks, int nblocks,
                             const shq_io_conv *conv, void *const d_out[])
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    SHQ_CHECK(ptype >= 0 && ptype < 6, SHQ_ERR_INVALID, "io_gather: ptype %d", ptype);
    SHQ_TRY(check_layout(layout, d_parts, numpart, false));
    SHQ_CHECK(n >= 0 && n < (1ll << 31) - 64 && (d_selection || n == 0), SHQ_ERR_INVALID, "io_gather: bad selection");
    bool need_slot = false;
    SHQ_TRY(check_blocks(layout, ptype, blocks, nblocks, (const void *const *) d_out, n, &need_slot));
    if(need_slot)
        SHQ_TRY(check_slots(layout, ptype, d_slots, slot_size));
    SHQ_TRY(check_conv(conv, blocks, nblocks, true));
    if(n == 0 || nblocks == 0)
        return SHQ_OK;
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    SHQ_TRY(io_reset(ctx));
    const IoRec pr = io_rec(layout, d_parts, numpart);
    const size_t ses = need_slot ? layout->slot_elsize[ptype] : 0;
    const unsigned pb = (unsigned) io_pitch(layout->part_elsize), ps = need_slot ? (unsigned) io_pitch(ses) : 0;
    const int wide_base = layout->part_elsize % 16 == 0 && (uintptr_t) d_parts % 16 == 0;
    const int wide_slot = need_slot && ses % 16 == 0 && (uintptr_t) d_slots[ptype] % 16 == 0;
    for(int b0 = 0; b0 < nblocks; b0 += SHQ_IO_MAXBLOCKS) {
        IoBlocks B;
        memset(&B, 0, sizeof(B));
        B.n = std::min(nblocks - b0, (int) SHQ_IO_MAXBLOCKS);
        bool slot_here = false;
        for(int b = 0; b < B.n; b++) {
            B.b[b] = blocks[b0 + b];
            B.col[b] = (char *) d_out[b0 + b];
            slot_here = slot_here || B.b[b].source == SHQ_IO_SRC_SLOT;
        }
        const size_t lds = (size_t) IO_TILE * std::max(pb, slot_here ? ps : 0u);
        io_gather_kernel<<<dim3(nblk(n, IO_TILE)), dim3(IO_TILE), lds, st>>>(pr, slot_here ? (const char *) d_slots[ptype] : nullptr, (unsigned) ses,
                                                                            slot_here ? (long long) slot_size[ptype] : 0ll, ptype, d_selection, (long long) n, B, *conv,
                                                                            slot_here ? 1 : 0, pb, ps, wide_base, wide_slot, io_err(ctx), reinterpret_cast<const char *>(ctx->io_cnt.ptr));
        SHQ_HIP(hipGetLastError());
    }
    int e = 0;
    SHQ_HIP(hipMemcpyAsync(&e, io_err(ctx), sizeof(e), hipMemcpyDeviceToHost, st));
    SHQ_HIP(hipStreamSynchronize(st));
    SHQ_CHECK(!(e & IO_E_INDEX), SHQ_ERR_INVALID, "io_gather: a selection entry lies outside [0, %ld)", (long) numpart);
    SHQ_CHECK(!(e & IO_E_TYPE), SHQ_ERR_INVALID, "io_gather: a selected particle has a Type other than %d", ptype);
    SHQ_CHECK(!(e & IO_E_PI), SHQ_ERR_INVALID, "io_gather: a PI lies outside the slot array of type %d", ptype);
    SHQ_CHECK(!(e & IO_E_POSITION), SHQ_ERR_INVALID, "io_gather: a position is not finite or further than 64 boxes away");
    return SHQ_OK;
}

extern "C" int shq_io_scatter(shq_context *ctx, const shq_io_layout *layout, void *d_parts, int64_t numpart, void *const d_slots[6], const int64_t slot_size[6],
                              int ptype, int64_t n, const shq_io_block *blocks, int nblocks, const shq_io_conv *conv, const void *const d_in[])
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    SHQ_CHECK(ptype >= 0 && ptype < 6, SHQ_ERR_INVALID, "io_scatter: ptype %d", ptype);
    SHQ_TRY(check_layout(layout, d_parts, numpart, false));
    SHQ_CHECK(n >= 0, SHQ_ERR_INVALID, "io_scatter: n = %ld", (long) n);
    bool need_slot = false;
    SHQ_TRY(check_blocks(layout, ptype, blocks, nblocks, d_in, n, &need_slot));
    if(need_slot)
        SHQ_TRY(check_slots(layout, ptype, (const void *const *) d_slots, slot_size));
    SHQ_TRY(check_conv(conv, blocks, nblocks, false));
    int64_t cnt = 0;
    const IoRec pr = io_rec(layout, d_parts, numpart);
    hipStream_t st = ctx->stream;
    if(numpart > 0) {
        SHQ_HIP(hipSetDevice(ctx->device));
        SHQ_TRY(io_reset(ctx));
        SHQ_TRY(ctx->io_u8[0].reserve((size_t) numpart));
        SHQ_TRY(ctx->io_i32.reserve((size_t) numpart));
        io_typeflag_kernel<<<dim3(nblk(numpart)), dim3(256), 0, st>>>(pr, ptype, ctx->io_u8[0].ptr);
        SHQ_HIP(hipGetLastError());
        SHQ_TRY(prim_select_flagged(ctx, rocprim::counting_iterator<int32_t>(0), ctx->io_u8[0].ptr, ctx->io_i32.ptr, (size_t) numpart, ctx->io_cnt.ptr + 9, &cnt));
    }
    SHQ_CHECK(cnt == n, SHQ_ERR_INVALID, "io_scatter: %ld rows for %ld particles of type %d", (long) n, (long) cnt, ptype);
    if(cnt == 0 || nblocks == 0)
        return SHQ_OK;
    if(need_slot) {
        io_scatter_check_kernel<<<dim3(nblk(cnt)), dim3(256), 0, st>>>(pr, ctx->io_i32.ptr, cnt, (long long) slot_size[ptype], io_err(ctx));
        SHQ_HIP(hipGetLastError());
        int e = 0;
        SHQ_HIP(hipMemcpyAsync(&e, io_err(ctx), sizeof(e), hipMemcpyDeviceToHost, st));
        SHQ_HIP(hipStreamSynchronize(st));
        SHQ_CHECK(e == 0, SHQ_ERR_INVALID, "io_scatter: a PI lies outside the slot array of type %d", ptype);
    }
    for(int b0 = 0; b0 < nblocks; b0 += SHQ_IO_MAXBLOCKS) { /* chunks in array order on one stream: the order per particle holds */
        IoBlocks B;
        memset(&B, 0, sizeof(B));
        B.n = std::min(nblocks - b0, (int) SHQ_IO_MAXBLOCKS);
        for(int b = 0; b < B.n; b++) {
            B.b[b] = blocks[b0 + b];
            B.col[b] = (char *) d_in[b0 + b];
        }
        io_scatter_kernel<<<dim3(nblk(cnt)), dim3(256), 0, st>>>(pr, (char *) d_parts, need_slot ? (char *) d_slots[ptype] : nullptr,
                                                                need_slot ? layout->slot_elsize[ptype] : 0, ctx->io_i32.ptr, cnt, B, *conv);
        SHQ_HIP(hipGetLastError());
    }
    return SHQ_OK;
}
