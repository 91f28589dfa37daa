/* zeldovich.hip — the initial-condition displacements on the device for one rank: displacement_fields (libgenic/zeldovich.cpp:150-264)
 * with gaussian_fill / pmic_fill_gaussian_gadget (zeldovich.cpp:362-383, libgenic/pmesh.h:64-178), the seven transfer functions
 * (zeldovich.cpp:277-334), petapm's CIC readout (pm_iterate_one, petapm.cpp:1133-1183) and the final particle loop.
 *
 * The Gaussian field.  pmesh.h seeds one mt19937 per mesh column (i, j) from a table of seeds and draws a serial stream along k.  Both of
 * its generators advance one SAMPLE per k whichever is drawn first, so the mode (i, j, k) is the k-th SAMPLE of the generator seeded with
 * table[0][0][i, j] - except in the columns with d1 = d2 = 1 at k = 0 and k = Nmesh / 2, where it is the conjugate of the k-th SAMPLE of the
 * generator seeded with table[1][1][i, j].  So zel_fill_kernel runs ONE generator per column, and a second launch of the same kernel
 * (PATCH) runs the table[1][1] generator of the d = 1 columns and rewrites their two planes.  Both launches work on a range of columns and
 * read nothing outside it, so a slab can be cut from them.
 *  - One lane per column: init_genrand is a 624-step serial recurrence, so the parallelism is across columns.
 *  - The 624-word state of a lane lives in a device workspace laid out word-major ([word][lane]): the 64 lanes of a wave read or write
 *    word w in one 256-byte line.  A draw is generated as it is consumed (new mt[i] from mt[i], mt[i + 1], mt[i + 397], then tempered),
 *    which is the block twist taken one word at a time: two loads and one store of 4 bytes per draw, mt[i + 1] carried in a register.
 *    (64 lane-private states would fill the CU's 160 KiB of LDS to the byte for one wave; the workspace costs no occupancy.)
 *  - A wave collects 64 columns x 8 modes in LDS and stores them as 128-byte runs along k.
 * The spectrum is written in the dense [x][y][z'] layout that the transfer kernels read, pmesh's (i, j, k) = petapm's (x, y, z') by the
 * axis permutation of gaussian_fill; it stays resident in the context, keyed on (Nmesh, Seed, UnitaryAmplitude, InvertPhase).
 *
 * Per field: one kernel applies the transfer function to the resident spectrum into the call's work mesh, the c2r runs in place
 * (the bespoke pipeline of fft3d.hip where it has the mesh size, hipFFT otherwise), one kernel gathers the mesh at the particles with
 * pm_iterate_one's weights.  A last kernel does the particle loop and the two max reductions.
 * The call owns every buffer it uses; of the context it touches only the resident field and the FFT twiddle table.
 *
 * Several ranks: the same phases as entry points of their own (shq_zeldovich_slab_*, at the end of the file) on the caller's device
 * memory, with the caller's exchanges between them (shenqi_amd/dist.py, DistZeldovich).  The fill takes the columns (i, j) of a rank's
 * y-slab, so no Gaussian field travels; the transfer is fused into the X inverse of that slab (fft3d.hip, fft_pass_strided MODE 6) with
 * zel_transfer_mode, the function zel_transfer_kernel applies; the gather reads a window of x planes.
 */
#include "mesh_common.hpp"
#include <math.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>

namespace {

/* libm through pointers the compiler cannot see through: exp and sqrt as the reference calls them */
double (*volatile libm_exp)(double) = exp;
double (*volatile libm_sqrt)(double) = sqrt;

constexpr int ZW = 64;                /* fill: one wave per workgroup, one column per lane */
constexpr int ZK = 8;                 /* modes per column in one LDS tile: 8 x 16 bytes = one 128-byte run along k */
constexpr int ZT = 256;               /* the per-mode and per-particle kernels */
constexpr int MT_N = 624, MT_M = 397;
constexpr long long ZEL_CHUNK = 131072; /* columns per fill launch: 2,496 bytes of workspace each */

/* mt19937 with the state in a strided workspace: word w of this lane's generator is st[w * stride] */
struct MtLane {
    uint32_t *st;
    size_t stride;
    int i;        /* the next word to regenerate */
    uint32_t cur; /* mt[i] */
};

__device__ __forceinline__ void mt_seed(MtLane &g, uint32_t seed)
{
    uint32_t s = seed;
    g.st[0] = s;
    for(int w = 1; w < MT_N; w++) {
        s = 1812433253u * (s ^ (s >> 30)) + (uint32_t) w;
        g.st[(size_t) w * g.stride] = s;
    }
    g.i = 0;
    g.cur = seed;
}

/* a state as it is before its first twist */
__device__ __forceinline__ void mt_load(MtLane &g, const uint32_t *__restrict__ state)
{
    for(int w = 0; w < MT_N; w++)
        g.st[(size_t) w * g.stride] = state[w];
    g.i = 0;
    g.cur = state[0];
}

__device__ __forceinline__ uint32_t mt_draw(MtLane &g)
{
    const int i = g.i;
    const int i1 = i + 1 == MT_N ? 0 : i + 1;
    const int im = i + MT_M >= MT_N ? i + MT_M - MT_N : i + MT_M;
    const uint32_t nx = g.st[(size_t) i1 * g.stride];
    const uint32_t y = (g.cur & 0x80000000u) | (nx & 0x7fffffffu);
    uint32_t v = g.st[(size_t) im * g.stride] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    g.st[(size_t) i * g.stride] = v;
    g.i = i1;
    g.cur = nx;
    v ^= v >> 11;
    v ^= (v << 7) & 0x9d2c5680u;
    v ^= (v << 15) & 0xefc60000u;
    v ^= v >> 18;
    return v;
}

/* SAMPLE (pmesh.h:55-62) with boost's uniform_real_distribution(0, 1) on a 32-bit engine: draw / 2^32 */
__device__ __forceinline__ void mt_sample(MtLane &g, double *ampl, double *phase)
{
#pragma clang fp contract(off)
    *phase = ((double) mt_draw(g) / 4294967296.0) * 2 * M_PI;
    double a;
    do
        a = (double) mt_draw(g) / 4294967296.0;
    while(a == 0);
    *ampl = a;
}

/* pmic_fill_gaussian_gadget's column loop (pmesh.h:93-172) for the columns [c0, c1) of a y-slab: c = i * njl + jl is the column (i, j)
 * with j = j0 + jl, and its modes are stored as row c of `spec`, `pitch` complex apart (the whole mesh: j0 = 0, njl = N, pitch =
 * N / 2 + 1).  The seed tables are the whole mesh's, [N][N].  Pad columns k > N / 2 of a wider pitch are written as 0.
 * !PATCH: tab = table[0][0]; every mode of the column from its own generator, the self-conjugate modes real, the zero mode 0.
 *  PATCH: tab = table[1][1]; the d1 = d2 = 1 columns only, their k = 0 and k = N / 2 modes conjugated (launched after the other). */
template <bool PATCH>
__global__ __launch_bounds__(ZW) void zel_fill_kernel(int N, long long c0, long long c1, int j0, int njl, int pitch, const uint32_t *__restrict__ tab,
                                                      uint32_t *ws, int unitary, int invert, double2 *__restrict__ spec)
{
#pragma clang fp contract(off)
    __shared__ double2 tile[ZW][ZK + 1];
    const int lane = threadIdx.x;
    const long long cbase = c0 + (long long) blockIdx.x * ZW;
    const long long c = cbase + lane;
    const int Nc = N / 2 + 1;
    bool act = c < c1;
    const int i = act ? (int) (c / njl) : 0, j = j0 + (act ? (int) (c - (long long) i * njl) : 0);
    const int ci = (N - i) % N, cj = (N - j) % N;
    const bool d = (ci == i && cj < j) || ci < i; /* pmesh.h:109-114 */
    if(PATCH)
        act = act && d;
    MtLane g;
    g.stride = (size_t) gridDim.x * ZW;
    g.st = ws + (size_t) blockIdx.x * ZW + lane;
    if(act)
        mt_seed(g, tab[(size_t) i * N + j]);
    if(PATCH) {
        if(!act)
            return;
        for(int k = 0; k < Nc; k++) {
            double ampl, phase;
            mt_sample(g, &ampl, &phase);
            if(k != 0 && k != N / 2)
                continue;
            ampl = sqrt(-log(ampl));
            if(unitary)
                ampl = 1.0;
            if(invert)
                phase += M_PI;
            spec[(size_t) c * pitch + k] = make_double2(ampl * cos(phase), -(ampl * sin(phase)));
        }
        return;
    }
    const bool selfij = ci == i && cj == j;
    for(int k0 = 0; k0 < pitch; k0 += ZK) {
        if(act)
            for(int kk = 0; kk < ZK && k0 + kk < pitch; kk++) {
                const int k = k0 + kk;
                double2 v = make_double2(0.0, 0.0);
                if(k < Nc) {
                    double ampl, phase;
                    mt_sample(g, &ampl, &phase);
                    ampl = sqrt(-log(ampl));
                    if(unitary)
                        ampl = 1.0;
                    if(invert)
                        phase += M_PI;
                    v = make_double2(ampl * cos(phase), ampl * sin(phase));
                    if(selfij && (N - k) % N == k)
                        v.y = 0;
                    if(i == 0 && j == 0 && k == 0)
                        v = make_double2(0.0, 0.0);
                }
                tile[lane][kk] = v;
            }
        __syncthreads();
        for(int r = 0; r < ZW / 8; r++) {
            const int col = r * 8 + (lane >> 3), kk = lane & 7;
            if(cbase + col < c1 && k0 + kk < pitch)
                spec[(size_t) (cbase + col) * pitch + k0 + kk] = tile[col][kk];
        }
        __syncthreads();
    }
}

/* shq_zeldovich_column_draws: per generator the first m outputs, and (restarted) the first m / 2 SAMPLEs */
__global__ __launch_bounds__(ZW) void zel_draws_kernel(int n, const uint32_t *__restrict__ seeds, const uint32_t *__restrict__ states, int m,
                                                       uint32_t *ws, uint32_t *__restrict__ raw, double *__restrict__ pairs)
{
    const int t = blockIdx.x * ZW + threadIdx.x;
    if(t >= n)
        return;
    MtLane g;
    g.stride = (size_t) gridDim.x * ZW;
    g.st = ws + t;
    for(int pass = 0; pass < 2; pass++) {
        if(states)
            mt_load(g, states + (size_t) t * MT_N);
        else
            mt_seed(g, seeds[t]);
        if(pass == 0)
            for(int q = 0; q < m; q++)
                raw[(size_t) t * m + q] = mt_draw(g);
        else
            for(int q = 0; q < m / 2; q++) {
                double ampl, phase;
                mt_sample(g, &ampl, &phase);
                pairs[((size_t) t * (m / 2) + q) * 2] = phase;
                pairs[((size_t) t * (m / 2) + q) * 2 + 1] = ampl;
            }
    }
}

/* dense [x][y][z'] -> the reference's Fourier layout [y][z'][x] (debug download) */
__global__ __launch_bounds__(ZT) void zel_layout_kernel(const double2 *__restrict__ in, double2 *__restrict__ out, int N, int Nc)
{
    const size_t total = (size_t) N * N * Nc;
    const size_t o = (size_t) blockIdx.x * ZT + threadIdx.x;
    if(o >= total)
        return;
    const int x = (int) (o % N), z = (int) ((o / N) % Nc), y = (int) (o / ((size_t) N * Nc));
    out[o] = in[((size_t) x * N + y) * Nc + z];
}

/* density_transfer / disp_transfer (zeldovich.cpp:277-314) from the resident spectrum [x][y][Nc] into the work mesh [x][y][zpc]:
 * axis < 0: value *= dens[k2] (the whole factor, made on the host);  else fac = c0 * kaxis / k2, fac *= tab[k2], value = i fac value */
__global__ __launch_bounds__(ZT) void zel_transfer_kernel(const double2 *__restrict__ spec, double2 *__restrict__ out, int N, int zpc,
                                                          const double *__restrict__ tab, int axis, double c0)
{
#pragma clang fp contract(off)
    const int Nc = N / 2 + 1;
    const size_t total = (size_t) N * N * Nc;
    const size_t ip = (size_t) blockIdx.x * ZT + threadIdx.x;
    if(ip >= total)
        return;
    const HalfMode md = half_mode(ip, N);
    const int kpos[3] = {md.kx, md.ky, md.z};
    out[md.row * zpc + md.z] = zel_transfer_mode(spec[ip], md.k2, axis < 0 ? 0 : kpos[axis], axis, md.k2 ? tab[md.k2] : 0.0, c0);
}

/* the same factor on a rank's dense y-slab [x][row][N / 2 + 1], row = mesh row y0 + row (shq_zeldovich_slab_transfer) */
__global__ __launch_bounds__(ZT) void zel_slab_transfer_kernel(const double2 *spec, double2 *out, int N, int y0, int nyl,
                                                               const double *__restrict__ tab, int axis, double c0)
{
#pragma clang fp contract(off)
    const int Nc = N / 2 + 1;
    const size_t total = (size_t) N * nyl * Nc;
    const size_t ip = (size_t) blockIdx.x * ZT + threadIdx.x;
    if(ip >= total)
        return;
    const int z = (int) (ip % Nc), row = (int) ((ip / Nc) % nyl), x = (int) (ip / ((size_t) Nc * nyl));
    const int y = y0 + row;
    const int kx = x <= N / 2 ? x : x - N, ky = y <= N / 2 ? y : y - N;
    const long long k2 = (long long) kx * kx + (long long) ky * ky + (long long) z * z;
    const int kpos[3] = {kx, ky, z};
    out[ip] = zel_transfer_mode(spec[ip], k2, axis < 0 ? 0 : kpos[axis], axis, k2 ? tab[k2] : 0.0, c0);
}

/* pm_iterate_one (petapm.cpp:1153-1177) with the readout functions: out[p] = sum over the 8 connections, in their order, of weight * mesh */
__global__ __launch_bounds__(ZT) void zel_readout_kernel(long long n, const double *__restrict__ pos, const double *__restrict__ mesh, int N,
                                                         int zp, double cellsize, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const long long p = (long long) blockIdx.x * ZT + threadIdx.x;
    if(p >= n)
        return;
    /* positions are in [0, BoxSize), so the cell is in [0, N]: N itself where Pos / CellSize rounds up to N, which is cell 0 with
     * residual 0 (the region's padding cells are the periodic images) */
    int ic[3];
    double res[3];
    cic_cell3(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], cellsize, N, ic, res);
    double acc = 0;
    cic_corners(ic, res, N, zp, [&](int, size_t lin, double weight) {
#pragma clang fp contract(off)
        acc += weight * mesh[lin];
    });
    out[p] = acc;
}

/* zel_readout_kernel on a rank's window [nalloc][N][zp] of x planes whose plane 0 is the mesh plane plane0: the same eight
 * connections in the same order with the same weights.  A particle with a corner outside the window raises *oob and writes nothing. */
__global__ __launch_bounds__(ZT) void zel_gather_kernel(long long n, const double *__restrict__ pos, const double *__restrict__ mesh, int N, int zp,
                                                        double cellsize, int plane0, int nalloc, double *__restrict__ out, int *oob)
{
#pragma clang fp contract(off)
    const long long p = (long long) blockIdx.x * ZT + threadIdx.x;
    if(p >= n)
        return;
    int ic[3];
    double res[3];
    cic_cell3(pos[3 * p], pos[3 * p + 1], pos[3 * p + 2], cellsize, N, ic, res);
    double acc = 0;
    int outside = 0;
    cic_corners<true>(
        ic, res, N, zp,
        [&](int, size_t lin, double weight) {
#pragma clang fp contract(off)
            acc += weight * mesh[lin];
        },
        plane0, nalloc, &outside);
    if(outside)
        *oob = 1;
    else
        out[p] = acc;
}

__device__ __forceinline__ double zel_wrap(double x, double L)
{
#pragma clang fp contract(off)
    for(int k = 0; x >= L && k < (1 << 20); k++)
        x -= L;
    for(int k = 0; x < 0 && k < (1 << 20); k++)
        x += L;
    return x;
}

/* the particle loop of displacement_fields (zeldovich.cpp:233-256); fld = [7][n]: Density, Disp x y z, Vel x y z.
 * mx[0]: the largest signed Disp component (from 0), mx[1]: the largest |Vel|^2; both >= 0, so their bit patterns order as integers */
__global__ __launch_bounds__(ZT) void zel_finalize_kernel(long long n, const double *__restrict__ pos, const double *__restrict__ fld, int scaledep,
                                                          double vel_prefac, double L, double *__restrict__ pos_out, double *__restrict__ vel_out,
                                                          double *__restrict__ disp_out, unsigned long long *mx)
{
#pragma clang fp contract(off)
    __shared__ unsigned long long s[2];
    if(threadIdx.x < 2)
        s[threadIdx.x] = 0;
    __syncthreads();
    const long long p = (long long) blockIdx.x * ZT + threadIdx.x;
    double maxdisp = 0, absv = 0;
    if(p < n) {
        for(int k = 0; k < 3; k++) {
            const double dis = fld[(size_t) (1 + k) * n + p];
            if(dis > maxdisp)
                maxdisp = dis;
            double x = pos[3 * p + k];
            x += dis;
            double v = scaledep ? fld[(size_t) (4 + k) * n + p] : dis;
            v *= vel_prefac;
            absv += v * v;
            pos_out[3 * p + k] = zel_wrap(x, L);
            vel_out[3 * p + k] = v;
            disp_out[3 * p + k] = dis;
        }
    }
    if(!(absv > 0))
        absv = 0; /* the reference's `absv > maxvel` never takes a NaN */
    atomicMax(&s[0], (unsigned long long) __double_as_longlong(maxdisp));
    atomicMax(&s[1], (unsigned long long) __double_as_longlong(absv));
    __syncthreads();
    if(threadIdx.x < 2 && s[threadIdx.x])
        atomicMax(&mx[threadIdx.x], s[threadIdx.x]);
}

/* SETSEED and the eight loops of pmesh.h:18-41, 81-90 on one rank (ORegion = the whole mesh) */
void zel_seed_table(int N, int Seed, uint32_t *t00, uint32_t *t11)
{
#pragma clang fp contract(off)
    std::mt19937 rng((uint32_t) Seed);
    memset(t00, 0, sizeof(uint32_t) * (size_t) N * N);
    memset(t11, 0, sizeof(uint32_t) * (size_t) N * N);
    auto setseed = [&](int i, int j) {
        const double u = (double) (uint32_t) rng() / 4294967296.0;
        const unsigned int seed = static_cast<unsigned int>(0x7fffffff * u);
        const int ii[2] = {i, (N - i) % N}, jj[2] = {j, (N - j) % N};
        t00[(size_t) ii[0] * N + jj[0]] = seed;
        t11[(size_t) ii[1] * N + jj[1]] = seed;
    };
    for(int i = 0; i < N / 2; i++) {
        int j;
        for(j = 0; j < i; j++) setseed(i, j);
        for(j = 0; j < i + 1; j++) setseed(j, i);
        for(j = 0; j < i; j++) setseed(N - 1 - i, j);
        for(j = 0; j < i + 1; j++) setseed(N - 1 - j, i);
        for(j = 0; j < i; j++) setseed(i, N - 1 - j);
        for(j = 0; j < i + 1; j++) setseed(j, N - 1 - i);
        for(j = 0; j < i; j++) setseed(N - 1 - i, N - 1 - j);
        for(j = 0; j < i + 1; j++) setseed(N - 1 - j, N - 1 - i);
    }
}

/* The two fill launches over the columns (i, j), j0 <= j < j0 + njl, into spec = [N][njl][pitch] complex, in chunks of the context's
 * fill chunk.  The seed tables are made here, for the whole mesh: every rank makes the same ones. */
int zel_fill_columns(shq_context *ctx, int N, int Seed, int unitary, int invert, int j0, int njl, int pitch, double2 *spec)
{
    const size_t NN = (size_t) N * N;
    std::vector<uint32_t> t00(NN), t11(NN);
    zel_seed_table(N, Seed, t00.data(), t11.data());
    CallScope sc(ctx, "zeldovich");
    const long long ncol = (long long) N * njl;
    long long chunk = ctx->zel_chunk > 0 ? ctx->zel_chunk : ZEL_CHUNK;
    chunk = std::min(ncol, (chunk + ZW - 1) / ZW * ZW);
    uint32_t *d_t00, *d_t11, *d_ws;
    SHQ_TRY(sc.alloc(&d_t00, NN));
    SHQ_TRY(sc.alloc(&d_t11, NN));
    SHQ_TRY(sc.alloc(&d_ws, (size_t) ((chunk + ZW - 1) / ZW * ZW) * MT_N));
    hipStream_t s = ctx->stream;
    SHQ_HIP(hipMemcpyAsync(d_t00, t00.data(), sizeof(uint32_t) * NN, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(d_t11, t11.data(), sizeof(uint32_t) * NN, hipMemcpyHostToDevice, s));
    for(int pass = 0; pass < 2; pass++)
        for(long long c0 = 0; c0 < ncol; c0 += chunk) {
            const long long c1 = std::min(ncol, c0 + chunk);
            const dim3 grid(nblk(c1 - c0, ZW));
            if(pass == 0)
                zel_fill_kernel<false><<<grid, dim3(ZW), 0, s>>>(N, c0, c1, j0, njl, pitch, d_t00, d_ws, unitary, invert, spec);
            else
                zel_fill_kernel<true><<<grid, dim3(ZW), 0, s>>>(N, c0, c1, j0, njl, pitch, d_t11, d_ws, unitary, invert, spec);
            SHQ_HIP(hipGetLastError());
        }
    SHQ_HIP(hipStreamSynchronize(s)); /* the host tables go out of scope */
    return SHQ_OK;
}

/* the resident field of (N, Seed, unitary, invert): reused, or filled; *filled says which */
int zel_ensure_field(shq_context *ctx, int N, int Seed, int unitary, int invert, bool *filled)
{
    *filled = false;
    if(ctx->zel_have && ctx->zel_n == N && ctx->zel_seed == Seed && ctx->zel_unitary == unitary && ctx->zel_invert == invert)
        return SHQ_OK;
    ctx->zel_have = false;
    const int Nc = N / 2 + 1;
    SHQ_TRY(ctx->zel_spec.reserve((size_t) N * N * Nc * 2));
    SHQ_TRY(zel_fill_columns(ctx, N, Seed, unitary, invert, 0, N, Nc, reinterpret_cast<double2 *>(ctx->zel_spec.ptr)));
    ctx->zel_have = true;
    ctx->zel_n = N;
    ctx->zel_seed = Seed;
    ctx->zel_unitary = unitary;
    ctx->zel_invert = invert;
    *filled = true;
    return SHQ_OK;
}

/* the factor tables by k2 (zeldovich.cpp:277-309): dens[k2] = exp(-k2 r2) * (Delta / sqrt(L^3)); c0 = 1 / (2 pi) / sqrt(L) */
void zel_density_table(int N, double L, const double *delta, double *dens)
{
#pragma clang fp contract(off)
    const long long nk2 = 3ll * (N / 2) * (N / 2) + 1;
    double r2 = 1.0 / N;
    r2 *= r2;
    dens[0] = 0;
    for(long long k2 = 1; k2 < nk2; k2++) {
        double fac = libm_exp(-k2 * r2);
        fac *= delta[k2] / libm_sqrt(L * L * L);
        dens[k2] = fac;
    }
}

} // namespace

/* ---- C-ABI ------------------------------------------------------------------------------ */

extern "C" int shq_zeldovich_seed_table(int Nmesh, int Seed, uint32_t *table00, uint32_t *table11)
{
    SHQ_CHECK(table00 && table11, SHQ_ERR_INVALID, "zeldovich: null argument");
    SHQ_TRY(mesh_check_size(Nmesh, "zeldovich"));
    zel_seed_table(Nmesh, Seed, table00, table11);
    return SHQ_OK;
}

extern "C" int shq_zeldovich_factor_tables(int Nmesh, double BoxSize, const double *delta, const double *growth, double *dens_fac,
                                           double *disp_fac, double *vel_fac)
{
#pragma clang fp contract(off)
    SHQ_CHECK(delta && dens_fac && disp_fac && (!vel_fac || growth), SHQ_ERR_INVALID, "zeldovich: null argument");
    SHQ_TRY(mesh_check_size(Nmesh, "zeldovich"));
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0, SHQ_ERR_INVALID, "zeldovich: BoxSize must be finite and > 0");
    const long long nk2 = 3ll * (Nmesh / 2) * (Nmesh / 2) + 1;
    zel_density_table(Nmesh, BoxSize, delta, dens_fac);
    disp_fac[0] = 0;
    if(vel_fac)
        vel_fac[0] = 0;
    for(long long k2 = 1; k2 < nk2; k2++) {
        const double fac = 1. / (2 * M_PI) / libm_sqrt(BoxSize) / k2;
        disp_fac[k2] = fac * delta[k2];
        if(vel_fac)
            vel_fac[k2] = fac * growth[k2];
    }
    return SHQ_OK;
}

extern "C" int shq_zeldovich_set_fill_chunk(shq_context *ctx, int64_t ncolumns)
{
    SHQ_CHECK(ctx && ncolumns >= 0 && ncolumns <= (1ll << 22), SHQ_ERR_INVALID, "zeldovich: fill chunk %lld outside [0, 2^22]", (long long) ncolumns);
    ctx->zel_chunk = ncolumns;
    return SHQ_OK;
}

extern "C" int shq_zeldovich_drop_field(shq_context *ctx)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    ctx->zel_have = false;
    ctx->zel_spec.release();
    return SHQ_OK;
}

extern "C" int shq_zeldovich_fill(shq_context *ctx, int Nmesh, int Seed, int UnitaryAmplitude, int InvertPhase)
{
    SHQ_CHECK(ctx, SHQ_ERR_INVALID, "null context");
    SHQ_TRY(mesh_check_size(Nmesh, "zeldovich"));
    SHQ_HIP(hipSetDevice(ctx->device));
    bool filled;
    return zel_ensure_field(ctx, Nmesh, Seed, UnitaryAmplitude != 0, InvertPhase != 0, &filled);
}

extern "C" int shq_zeldovich_download_field(shq_context *ctx, int Nmesh, double *complx)
{
    SHQ_CHECK(ctx && complx, SHQ_ERR_INVALID, "zeldovich: null argument");
    SHQ_CHECK(ctx->zel_have, SHQ_ERR_STATE, "zeldovich_download_field: no resident field (never filled, or dropped)");
    SHQ_CHECK(Nmesh == ctx->zel_n, SHQ_ERR_INVALID, "zeldovich_download_field: the resident field is %d^3, not %d^3", ctx->zel_n, Nmesh);
    SHQ_HIP(hipSetDevice(ctx->device));
    const int N = Nmesh, Nc = N / 2 + 1;
    const size_t modes = (size_t) N * N * Nc;
    CallScope sc(ctx, "zeldovich");
    double2 *d_out;
    SHQ_TRY(sc.alloc(&d_out, modes));
    zel_layout_kernel<<<dim3(nblk((long long) modes, ZT)), dim3(ZT), 0, ctx->stream>>>(reinterpret_cast<const double2 *>(ctx->zel_spec.ptr), d_out, N, Nc);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipMemcpyAsync(complx, d_out, sizeof(double2) * modes, hipMemcpyDeviceToHost, ctx->stream));
    SHQ_HIP(hipStreamSynchronize(ctx->stream));
    return SHQ_OK;
}

extern "C" int shq_zeldovich_phase_ms(shq_context *ctx, double ms[4])
{
    SHQ_CHECK(ctx && ms, SHQ_ERR_INVALID, "null argument");
    for(int i = 0; i < 4; i++)
        ms[i] = ctx->zel_ms[i];
    return SHQ_OK;
}

extern "C" int shq_zeldovich_column_draws(shq_context *ctx, int n, const uint32_t *seeds, const uint32_t *states, int m, uint32_t *raw,
                                          double *pairs)
{
    SHQ_CHECK(ctx && raw && pairs && (seeds || states), SHQ_ERR_INVALID, "zeldovich: null argument");
    SHQ_CHECK(n >= 1 && n <= 65536 && m >= 2 && m <= (1 << 20) && m % 2 == 0, SHQ_ERR_INVALID, "zeldovich_column_draws: n %d, m %d", n, m);
    SHQ_HIP(hipSetDevice(ctx->device));
    CallScope sc(ctx, "zeldovich");
    const unsigned nb = nblk(n, ZW);
    uint32_t *d_in, *d_ws, *d_raw;
    double *d_pairs;
    const size_t nin = states ? (size_t) n * MT_N : (size_t) n;
    SHQ_TRY(sc.alloc(&d_in, nin));
    SHQ_TRY(sc.alloc(&d_ws, (size_t) nb * ZW * MT_N));
    SHQ_TRY(sc.alloc(&d_raw, (size_t) n * m));
    SHQ_TRY(sc.alloc(&d_pairs, (size_t) n * m));
    hipStream_t s = ctx->stream;
    SHQ_HIP(hipMemcpyAsync(d_in, states ? states : seeds, sizeof(uint32_t) * nin, hipMemcpyHostToDevice, s));
    zel_draws_kernel<<<dim3(nb), dim3(ZW), 0, s>>>(n, states ? nullptr : d_in, states ? d_in : nullptr, m, d_ws, d_raw, d_pairs);
    SHQ_HIP(hipGetLastError());
    SHQ_HIP(hipMemcpyAsync(raw, d_raw, sizeof(uint32_t) * n * m, hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipMemcpyAsync(pairs, d_pairs, sizeof(double) * n * m, hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    return SHQ_OK;
}

extern "C" int shq_zeldovich_displacements(shq_context *ctx, const shq_zeldovich_params *p, const double *delta, const double *growth, int64_t n,
                                           const double *pos, double *pos_out, double *vel, double *density, double *disp, double *maxdisp,
                                           double *maxvel)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx && p && delta && pos_out && vel && density && maxdisp && maxvel, SHQ_ERR_INVALID, "zeldovich: null argument");
    /* ---- every check before anything is written */
    const int N = p->Nmesh;
    SHQ_TRY(mesh_check_size(N, "zeldovich"));
    const double L = p->BoxSize;
    SHQ_CHECK(isfinite(L) && L > 0 && isfinite(p->vel_prefac), SHQ_ERR_INVALID, "zeldovich: BoxSize must be finite and > 0, vel_prefac finite");
    const int scaledep = p->ScaleDepVelocity != 0;
    SHQ_CHECK(!scaledep || growth, SHQ_ERR_INVALID, "zeldovich: ScaleDepVelocity without a dlogGrowth table");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || pos), SHQ_ERR_INVALID, "zeldovich: %lld particles on one rank (< 2^31)", (long long) n);
    for(int64_t i = 0; i < 3 * n; i++) /* the reference ends the run: "particle out of cell" */
        SHQ_CHECK(pos[i] >= 0 && pos[i] < L, SHQ_ERR_INVALID, "zeldovich: particle %lld is outside [0, BoxSize): %g", (long long) (i / 3), pos[i]);
    const long long nk2 = 3ll * (N / 2) * (N / 2) + 1;
    for(long long k2 = 1; k2 < nk2; k2++)
        SHQ_CHECK(isfinite(delta[k2]) && (!scaledep || isfinite(growth[k2])), SHQ_ERR_INVALID, "zeldovich: non-finite table entry at k2 = %lld", k2);
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(shq_join_pm(ctx)); /* the bespoke transforms share the context's twiddle table with a prestarted PM */
    for(int i = 0; i < 4; i++)
        ctx->zel_ms[i] = 0;

    hipStream_t s = ctx->stream;
    CallScope sc(ctx, "zeldovich");
    SHQ_TRY(sc.mark(s));
    bool filled = false;
    SHQ_TRY(zel_ensure_field(ctx, N, p->Seed, p->UnitaryAmplitude != 0, p->InvertPhase != 0, &filled));
    SHQ_TRY(sc.mark(s)); /* ev[1]: the field is resident */

    /* ---- tables, particles, the work mesh */
    std::vector<double> dens((size_t) nk2);
    zel_density_table(N, L, delta, dens.data());
    const double c0 = 1. / (2 * M_PI) / libm_sqrt(L);
    Fft3dRoute route = fft3d_route(N);
    const int zp = route.zp;
    const size_t padded = route.padded;
    const int nfields = scaledep ? 7 : 4;
    double *d_dens, *d_delta, *d_growth = nullptr, *d_mesh, *d_pos, *d_fld, *d_out;
    unsigned long long *d_mx;
    SHQ_TRY(sc.alloc(&d_dens, (size_t) nk2));
    SHQ_TRY(sc.alloc(&d_delta, (size_t) nk2));
    if(scaledep)
        SHQ_TRY(sc.alloc(&d_growth, (size_t) nk2));
    SHQ_TRY(sc.alloc(&d_mesh, padded));
    SHQ_TRY(sc.alloc(&d_pos, (size_t) 3 * n));
    SHQ_TRY(sc.alloc(&d_fld, (size_t) 7 * n));
    SHQ_TRY(sc.alloc(&d_out, (size_t) 9 * n)); /* Pos, Vel, Disp */
    SHQ_TRY(sc.alloc(&d_mx, 2));
    SHQ_HIP(hipMemcpyAsync(d_dens, dens.data(), sizeof(double) * nk2, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemcpyAsync(d_delta, delta, sizeof(double) * nk2, hipMemcpyHostToDevice, s));
    if(scaledep)
        SHQ_HIP(hipMemcpyAsync(d_growth, growth, sizeof(double) * nk2, hipMemcpyHostToDevice, s));
    if(n > 0)
        SHQ_HIP(hipMemcpyAsync(d_pos, pos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, s));
    SHQ_HIP(hipMemsetAsync(d_mesh, 0, sizeof(double) * padded, s)); /* the pitch's padding is never written again */
    SHQ_HIP(hipMemsetAsync(d_mx, 0, sizeof(unsigned long long) * 2, s));
    SHQ_TRY(route_plans(sc, route, false, true));

    /* ---- per field: transfer, c2r, readout (zeldovich.cpp:183-192: Density, DispX/Y/Z, VelX/Y/Z) */
    const size_t modes = (size_t) N * N * (N / 2 + 1);
    const double cellsize = L / N;
    for(int f = 0; f < nfields; f++) {
        const int axis = f == 0 ? -1 : (f - 1) % 3;
        const double *tab = f == 0 ? d_dens : (f < 4 ? d_delta : d_growth);
        zel_transfer_kernel<<<dim3(nblk((long long) modes, ZT)), dim3(ZT), 0, s>>>(reinterpret_cast<const double2 *>(ctx->zel_spec.ptr),
                                                                      reinterpret_cast<double2 *>(d_mesh), N, zp / 2, tab, axis, c0);
        SHQ_HIP(hipGetLastError());
        SHQ_TRY(route_inverse(ctx, sc, route, d_mesh));
        if(n > 0)
            zel_readout_kernel<<<dim3(nblk(n, ZT)), dim3(ZT), 0, s>>>(n, d_pos, d_mesh, N, zp, cellsize, d_fld + (size_t) f * n);
        SHQ_HIP(hipGetLastError());
    }
    SHQ_TRY(sc.mark(s)); /* ev[2]: the fields are read out */

    /* ---- the particle loop and the two maxima */
    if(n > 0)
        zel_finalize_kernel<<<dim3(nblk(n, ZT)), dim3(ZT), 0, s>>>(n, d_pos, d_fld, scaledep, p->vel_prefac, L, d_out, d_out + 3 * n,
                                                                           d_out + 6 * n, d_mx);
    SHQ_HIP(hipGetLastError());
    SHQ_TRY(sc.mark(s)); /* ev[3]: the particle loop */
    unsigned long long mx[2] = {0, 0};
    SHQ_HIP(hipMemcpyAsync(mx, d_mx, sizeof(mx), hipMemcpyDeviceToHost, s));
    if(n > 0) {
        SHQ_HIP(hipMemcpyAsync(pos_out, d_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        SHQ_HIP(hipMemcpyAsync(vel, d_out + 3 * n, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        SHQ_HIP(hipMemcpyAsync(density, d_fld, sizeof(double) * n, hipMemcpyDeviceToHost, s));
        if(disp)
            SHQ_HIP(hipMemcpyAsync(disp, d_out + 6 * n, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
    }
    SHQ_TRY(sc.mark(s)); /* ev[4]: downloaded */
    SHQ_HIP(hipStreamSynchronize(s));
    memcpy(maxdisp, &mx[0], sizeof(double));
    memcpy(maxvel, &mx[1], sizeof(double));
    ctx->zel_ms[0] = filled ? sc.ms(0, 1) : 0.0;
    ctx->zel_ms[1] = sc.ms(1, 2);
    ctx->zel_ms[2] = sc.ms(2, 3);
    ctx->zel_ms[3] = sc.ms(0, 4);
    return SHQ_OK;
}

/* ---- the same phases on a rank's slab (several ranks: shenqi_amd/dist.py, DistZeldovich) ---------------------------------------
 * Every pointer named d_ is device memory of the caller (torch tensors).  The Gaussian field lives on a y-slab [N][nyl][zpc] complex
 * (zpc = shq_zeldovich_slab_pitch / 2, or N / 2 + 1 without a bespoke transform), a field's real mesh on the rank's x planes
 * [nalloc][N][zp] doubles.  None of these calls reads or writes the PM's state or the one-rank resident field: the twiddles, the tables
 * and the flags are the context's zels_ ones. */
namespace {

/* the table and the axis of field 0 .. 6 (Density, DispX/Y/Z, VelX/Y/Z) from the uploaded tables */
int zel_slab_field(shq_context *ctx, int N, double BoxSize, int field, const char *who, const double **tab, int *axis)
{
    SHQ_CHECK(field >= 0 && field < 7, SHQ_ERR_INVALID, "%s: field %d outside [0, 7)", who, field);
    SHQ_CHECK(ctx->zels_tabs_n == N && ctx->zels_box == BoxSize, SHQ_ERR_STATE,
              "%s: no tables of mesh size %d and this BoxSize (shq_zeldovich_slab_tables first)", who, N);
    SHQ_CHECK(field < 4 || ctx->zels_growth, SHQ_ERR_STATE, "%s: a velocity field without a dlogGrowth table", who);
    const size_t nk2 = 3 * (size_t) (N / 2) * (N / 2) + 1;
    *tab = ctx->zels_tabs.ptr + (field == 0 ? 0 : (field < 4 ? 1 : 2)) * nk2;
    *axis = field == 0 ? -1 : (field - 1) % 3;
    return SHQ_OK;
}

} // namespace

extern "C" int shq_zeldovich_slab_pitch(int Nmesh) { return slab_pitch(Nmesh); }

extern "C" int shq_zeldovich_slab_fill(shq_context *ctx, int Nmesh, int Seed, int UnitaryAmplitude, int InvertPhase, int y0, int nyl, void *d_spec)
{
    SHQ_CHECK(ctx && d_spec, SHQ_ERR_INVALID, "zeldovich_slab_fill: null argument");
    SHQ_TRY(mesh_check_size(Nmesh, "zeldovich_slab_fill"));
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= Nmesh, SHQ_ERR_INVALID, "zeldovich_slab_fill: bad slab geometry");
    SHQ_HIP(hipSetDevice(ctx->device));
    const int zp = shq_zeldovich_slab_pitch(Nmesh);
    return zel_fill_columns(ctx, Nmesh, Seed, UnitaryAmplitude != 0, InvertPhase != 0, y0, nyl, zp ? zp / 2 : Nmesh / 2 + 1, (double2 *) d_spec);
}

extern "C" int shq_zeldovich_slab_tables(shq_context *ctx, int Nmesh, double BoxSize, const double *delta, const double *growth)
{
    SHQ_CHECK(ctx && delta, SHQ_ERR_INVALID, "zeldovich_slab_tables: null argument");
    const int N = Nmesh;
    SHQ_TRY(mesh_check_size(N, "zeldovich_slab_tables"));
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0, SHQ_ERR_INVALID, "zeldovich_slab_tables: BoxSize must be finite and > 0");
    const size_t nk2 = 3 * (size_t) (N / 2) * (N / 2) + 1;
    for(size_t k2 = 1; k2 < nk2; k2++)
        SHQ_CHECK(isfinite(delta[k2]) && (!growth || isfinite(growth[k2])), SHQ_ERR_INVALID, "zeldovich_slab_tables: non-finite table entry at k2 = %zu", k2);
    SHQ_HIP(hipSetDevice(ctx->device));
    std::vector<double> tabs(3 * nk2, 0.0);
    zel_density_table(N, BoxSize, delta, tabs.data());
    memcpy(tabs.data() + nk2, delta, sizeof(double) * nk2);
    if(growth)
        memcpy(tabs.data() + 2 * nk2, growth, sizeof(double) * nk2);
    tabs[nk2] = tabs[2 * nk2] = 0; /* entry 0 is what a pad column fetches: never used, but finite */
    ctx->zels_tabs_n = 0;
    SHQ_HIP(hipStreamSynchronize(ctx->stream)); /* a transfer pass may still read the previous tables */
    SHQ_TRY(ctx->zels_tabs.reserve(tabs.size()));
    SHQ_HIP(hipMemcpy(ctx->zels_tabs.ptr, tabs.data(), sizeof(double) * tabs.size(), hipMemcpyHostToDevice));
    ctx->zels_tabs_n = N;
    ctx->zels_growth = growth != nullptr;
    ctx->zels_box = BoxSize;
    return SHQ_OK;
}

/* The transfer pass of one field on the kept Gaussian field d_spec = [N][nyl][zp / 2] complex: zel_transfer_mode per mode, then the X
 * inverse, stored into d_out of the same shape.  d_spec is only read. */
extern "C" int shq_zeldovich_slab_xtransfer(shq_context *ctx, int Nmesh, double BoxSize, const void *d_spec, void *d_out, int y0, int nyl, int field)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx && d_spec && d_out && d_spec != d_out, SHQ_ERR_INVALID, "zeldovich_slab_xtransfer: null argument, or the pass asked to run in place");
    const int N = Nmesh, zp = shq_zeldovich_slab_pitch(N);
    SHQ_CHECK(zp > 0, SHQ_ERR_INVALID, "zeldovich_slab_xtransfer: mesh size %d has no bespoke FFT", N);
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= N, SHQ_ERR_INVALID, "zeldovich_slab_xtransfer: bad slab geometry");
    shq_fft_opts o;
    SHQ_TRY(zel_slab_field(ctx, N, BoxSize, field, "zeldovich_slab_xtransfer", &o.modefac, &o.zel_axis));
    SHQ_HIP(hipSetDevice(ctx->device));
    SHQ_TRY(slab_twiddles(ctx, ctx->zels_tw, ctx->zels_tw_n, N, &o.tw));
    o.nslab = nyl;
    o.y0 = y0;
    o.fac_mask = -1;
    o.out = (double *) d_out;
    o.zel_c0 = 1. / (2 * M_PI) / libm_sqrt(BoxSize);
    return shq_fft3d_run(ctx, (double *) const_cast<void *>(d_spec), N, zp, SHQ_FFT_X_ZEL, false, 1.0, nullptr, 0, 0, o);
}

/* the same factor for a mesh size without a bespoke transform, between the caller's own X transforms: d_spec = [N][nyl][N / 2 + 1]
 * complex, dense, x slowest, into d_out of the same shape (d_out may be d_spec) */
extern "C" int shq_zeldovich_slab_transfer(shq_context *ctx, int Nmesh, double BoxSize, const void *d_spec, void *d_out, int y0, int nyl, int field)
{
#pragma clang fp contract(off)
    SHQ_CHECK(ctx && d_spec && d_out, SHQ_ERR_INVALID, "zeldovich_slab_transfer: null argument");
    const int N = Nmesh;
    SHQ_TRY(mesh_check_size(N, "zeldovich_slab_transfer"));
    SHQ_CHECK(nyl > 0 && y0 >= 0 && y0 + nyl <= N, SHQ_ERR_INVALID, "zeldovich_slab_transfer: bad slab geometry");
    const double *tab;
    int axis;
    SHQ_TRY(zel_slab_field(ctx, N, BoxSize, field, "zeldovich_slab_transfer", &tab, &axis));
    SHQ_HIP(hipSetDevice(ctx->device));
    const long long modes = (long long) N * nyl * (N / 2 + 1);
    zel_slab_transfer_kernel<<<dim3(nblk(modes, ZT)), dim3(ZT), 0, ctx->stream>>>((const double2 *) d_spec, (double2 *) d_out, N, y0, nyl, tab, axis,
                                                                                 1. / (2 * M_PI) / libm_sqrt(BoxSize));
    SHQ_HIP(hipGetLastError());
    return SHQ_OK;
}

/* the Y/Z inverse of `nplanes` x planes [nplanes][N][zp] doubles, in place; d_packed (NULL: the planes hold the spectrum already) is the
 * all-to-all buffer [nranks][nplanes][N / nranks][zp / 2] complex the Y pass reads instead */
extern "C" int shq_zeldovich_slab_fft_yz(shq_context *ctx, int Nmesh, void *d_planes, int nplanes, const void *d_packed, int nranks)
{
    return slab_fft_yz(ctx, "zeldovich_slab_fft_yz", &shq_context::zels_tw, &shq_context::zels_tw_n, Nmesh, d_planes, nplanes, 1, SLAB_EXP_ONE, d_packed,
                       nranks);
}

/* pm_iterate_one's gather of d_mesh = [nalloc][N][zp] doubles (zp: the slab pitch, or N + 2 without a bespoke transform) at d_pos =
 * double[n][3] into d_out[n]: the rank's own planes from plane0 on and, for a slab with a neighbour, the neighbour's first plane
 * behind them (nalloc = nplanes + 1; nplanes = N: the whole periodic mesh, nalloc = N) */
extern "C" int shq_zeldovich_slab_gather(shq_context *ctx, int Nmesh, double BoxSize, const void *d_pos, int64_t n, const void *d_mesh, int plane0,
                                         int nplanes, int nalloc, void *d_out)
{
    SHQ_CHECK(ctx && d_mesh, SHQ_ERR_INVALID, "zeldovich_slab_gather: null argument");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_pos && d_out)), SHQ_ERR_INVALID, "zeldovich_slab_gather: bad particle arrays");
    const int N = Nmesh;
    SHQ_TRY(mesh_check_size(N, "zeldovich_slab_gather"));
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0, SHQ_ERR_INVALID, "zeldovich_slab_gather: BoxSize must be finite and > 0");
    SHQ_CHECK(slab_window_ok(N, plane0, nplanes, nalloc), SHQ_ERR_INVALID, "zeldovich_slab_gather: bad slab geometry");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SHQ_TRY(slab_flag_reset(ctx, ctx->zels_flag));
    if(n > 0)
        zel_gather_kernel<<<dim3(nblk(n, ZT)), dim3(ZT), 0, s>>>(n, (const double *) d_pos, (const double *) d_mesh, N, fft3d_route(N).zp,
                                                                  BoxSize / N, plane0, nalloc, (double *) d_out, ctx->zels_flag.ptr);
    SHQ_HIP(hipGetLastError());
    int oob;
    SHQ_TRY(slab_flag_read(ctx, ctx->zels_flag.ptr, &oob));
    SHQ_CHECK(!oob, SHQ_ERR_INVALID, "zeldovich_slab_gather: a particle lies outside this rank's slab (planes %d .. %d)", plane0, plane0 + nplanes - 1);
    return SHQ_OK;
}

/* the particle loop on device pointers: d_pos = double[n][3], d_fld = double[7][n] (rows 4 .. 6 read only with ScaleDepVelocity),
 * d_pos_out, d_vel, d_disp = double[n][3]; mx = this rank's maxdisp and max |Vel|^2 */
extern "C" int shq_zeldovich_slab_finalize(shq_context *ctx, int64_t n, const void *d_pos, const void *d_fld, int ScaleDepVelocity, double vel_prefac,
                                           double BoxSize, void *d_pos_out, void *d_vel, void *d_disp, double mx[2])
{
    SHQ_CHECK(ctx && mx, SHQ_ERR_INVALID, "zeldovich_slab_finalize: null argument");
    SHQ_CHECK(n >= 0 && n < (1ll << 31) && (n == 0 || (d_pos && d_fld && d_pos_out && d_vel && d_disp)), SHQ_ERR_INVALID,
              "zeldovich_slab_finalize: bad particle arrays");
    SHQ_CHECK(isfinite(BoxSize) && BoxSize > 0 && isfinite(vel_prefac), SHQ_ERR_INVALID,
              "zeldovich_slab_finalize: BoxSize must be finite and > 0, vel_prefac finite");
    SHQ_HIP(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    SHQ_TRY(ctx->zels_mx.reserve(2));
    SHQ_HIP(hipMemsetAsync(ctx->zels_mx.ptr, 0, sizeof(unsigned long long) * 2, s));
    if(n > 0)
        zel_finalize_kernel<<<dim3(nblk(n, ZT)), dim3(ZT), 0, s>>>(n, (const double *) d_pos, (const double *) d_fld, ScaleDepVelocity != 0, vel_prefac,
                                                                    BoxSize, (double *) d_pos_out, (double *) d_vel, (double *) d_disp, ctx->zels_mx.ptr);
    SHQ_HIP(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    SHQ_HIP(hipMemcpyAsync(h, ctx->zels_mx.ptr, sizeof(h), hipMemcpyDeviceToHost, s));
    SHQ_HIP(hipStreamSynchronize(s));
    memcpy(mx, h, sizeof(h));
    return SHQ_OK;
}
