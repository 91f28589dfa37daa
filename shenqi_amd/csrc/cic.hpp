/* cic.hpp — the cloud-in-cell pieces every mesh operator shares: the cell and residual of a position, and the eight corners of its cell
 * with their weights in pm_iterate_one's order (petapm.cpp:1147-1177). */
#pragma once
#include "common.hpp"

__device__ __forceinline__ int wrapi(int i, int N) { return i >= N ? i - N : (i < 0 ? i + N : i); }
/* x-plane index into the (possibly slab-local) mesh: global plane gx -> (gx - xshift) mod N.
 * xshift = 0 for the full periodic mesh; for a slab it is the global index of local plane 0. */
__device__ __forceinline__ int xloc(int gx, int xshift, int N)
{
    int v = (gx - xshift) % N;
    return v < 0 ? v + N : v;
}

/* CIC cell + residual: petapm.cpp:1147-1160 */
__device__ __forceinline__ void cic_setup(double p, double cell, int N, int &ic, double &res)
{
    const double tmp = p / cell; /* a true divide, as petapm.cpp:1148, so cells/weights match bit for bit */
    const double fl = floor(tmp);
    res = tmp - fl;
    int i = (int) fl;
    i %= N;
    if(i < 0)
        i += N;
    ic = i;
}

__device__ __forceinline__ void cic_cell3(double px, double py, double pz, double cell, int N, int ic[3], double res[3])
{
    cic_setup(px, cell, N, ic[0], res[0]);
    cic_setup(py, cell, N, ic[1], res[1]);
    cic_setup(pz, cell, N, ic[2], res[2]);
}

/* f(c, lin, w) for the connections c = 0..7 in order: bit k of c is the offset along axis k, lin the index of the periodic cell in a
 * mesh [N][N][zp], w the product of the three weights taken from 1.0 along k = 0, 1, 2.
 * SLAB: the mesh is a rank's window [nxalloc][N][zp] of x planes whose plane 0 is the global plane xshift (xloc above).  A corner whose
 * plane lies outside the window is not visited and raises *oob: the caller routed the particle to the wrong rank. */
template <bool SLAB = false, typename F>
__device__ __forceinline__ void cic_corners(const int ic[3], const double res[3], int N, int zp, F f, int xshift = 0, int nxalloc = 0,
                                            int *oob = nullptr)
{
#pragma clang fp contract(off)
#pragma unroll
    for(int c = 0; c < 8; c++) {
        double w = 1.0;
        size_t lin = 0;
        bool inside = true;
#pragma unroll
        for(int k = 0; k < 3; k++) {
            const int off = (c >> k) & 1;
            int t = wrapi(ic[k] + off, N);
            if(SLAB && k == 0) {
                t = xloc(t, xshift, N);
                inside = t < nxalloc;
            }
            lin = lin * (size_t) (k == 2 ? zp : N) + (size_t) t;
            w *= off ? res[k] : (1 - res[k]);
        }
        if(!SLAB || inside)
            f(c, lin, w);
        else
            *oob = 1;
    }
}
