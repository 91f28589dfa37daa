/* record_tile.hpp — the record-tile pass of startup.hip and stats.hip: a workgroup of ST_TILE threads owns ST_TILE consecutive particle
 * records and copies them between HBM and LDS with 16-byte (or 8-byte) pieces, consecutive lanes on consecutive pieces (the records are
 * contiguous, so this is a stream), ST_BATCH loads in flight per lane.  The LDS row pitch is the record size rounded up to an odd number
 * of 8-byte words (160 -> 168), so that lanes reading the same member of consecutive rows spread over the banks. */
#ifndef SHQ_RECORD_TILE_HPP
#define SHQ_RECORD_TILE_HPP
#include "common.hpp"

constexpr int ST_TILE = 256;
constexpr int ST_BATCH = 5;
constexpr size_t ST_MAXREC = 480;  /* slot records */
constexpr size_t ST_MAXPART = 240; /* particle records: ST_TILE * (240 + 8) bytes of LDS stay below the 64 KiB a launch gets without asking */

inline size_t st_pitch(size_t elsize) { return ((elsize / 8) & 1) ? elsize : elsize + 8; }

/* rows [0, nrow) of the tile at g (contiguous records of R bytes) into LDS rows of `pitch` bytes, CH bytes per lane and step */
template <int CH> __device__ __forceinline__ void st_stage_in(char *lds, unsigned pitch, const char *__restrict__ g, unsigned R, int nrow)
{
    const unsigned P = R / CH, total = (unsigned) nrow * P;
    for(unsigned t0 = threadIdx.x; t0 < total; t0 += ST_TILE * ST_BATCH) {
        uint4 v[ST_BATCH];
        unsigned dst[ST_BATCH];
#pragma unroll
        for(int u = 0; u < ST_BATCH; u++) {
            const unsigned t = t0 + (unsigned) u * ST_TILE;
            const bool in = t < total;
            const char *src = g + (size_t) (in ? t : 0u) * CH; /* piece 0 of the tile is always there */
            const unsigned rec = t / P;
            dst[u] = in ? rec * pitch + (t - rec * P) * CH : ~0u;
            if(CH == 16)
                v[u] = *reinterpret_cast<const uint4 *>(src);
            else {
                const uint2 w = *reinterpret_cast<const uint2 *>(src);
                v[u] = make_uint4(w.x, w.y, 0u, 0u);
            }
        }
#pragma unroll
        for(int u = 0; u < ST_BATCH; u++)
            if(dst[u] != ~0u) {
                uint2 *l = reinterpret_cast<uint2 *>(lds + dst[u]); /* the pitch keeps 8-byte alignment only */
                l[0] = make_uint2(v[u].x, v[u].y);
                if(CH == 16)
                    l[1] = make_uint2(v[u].z, v[u].w);
            }
    }
}

template <int CH> __device__ __forceinline__ void st_stage_out(const char *lds, unsigned pitch, char *__restrict__ g, unsigned R, int nrow)
{
    const unsigned P = R / CH, total = (unsigned) nrow * P;
    for(unsigned t = threadIdx.x; t < total; t += ST_TILE) {
        const unsigned rec = t / P;
        const uint2 *l = reinterpret_cast<const uint2 *>(lds + rec * pitch + (t - rec * P) * CH);
        if(CH == 16) {
            const uint2 a = l[0], b = l[1];
            *reinterpret_cast<uint4 *>(g + (size_t) t * CH) = make_uint4(a.x, a.y, b.x, b.y);
        } else
            *reinterpret_cast<uint2 *>(g + (size_t) t * CH) = l[0];
    }
}

#endif
